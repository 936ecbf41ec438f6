// Shared pieces of the fp32 fused MLP scorers (mlp_fused.hip: ncf_score_fused; mlp_topk.hip: ncf_mlp_topk): the packed-blob
// layout written by ncf_mlp_pack and the list of compiled (K0, N1, N2) instances.  Internal: not part of the ABI.
#pragma once
#include "ncf_common.h"

namespace ncf {

// blob layout (floats): Wp1[N1*K0] b1[N1] (Wp2[N2*N1] b2[N2])? wl[Nlast] bl[1] pad
struct BlobLayout {
    size_t wp1, b1, wp2, b2, wl, bl, total;
};
static BlobLayout blob_layout(const int* dims, int n_layers) {
    BlobLayout L{};
    const size_t K0 = dims[0], N1 = dims[1];
    size_t off = 0;
    L.wp1 = off; off += N1 * K0;
    L.b1 = off; off += N1;
    size_t last = N1;
    if (n_layers == 3) {
        const size_t N2 = dims[2];
        L.wp2 = off; off += N2 * N1;
        L.b2 = off; off += N2;
        last = N2;
    }
    L.wl = off; off += last;
    L.bl = off; off += 4;  // keep 16-byte granularity
    L.total = off;
    return L;
}

#define NCF_FUSED_INSTANCES(X) \
    X(64, 256, 128) X(64, 256, 0) X(64, 128, 0) X(64, 128, 64) \
    X(128, 256, 128) X(128, 256, 0) X(128, 128, 0) X(128, 128, 64) \
    X(256, 256, 128) X(256, 256, 0) X(256, 128, 0)

}  // namespace ncf
