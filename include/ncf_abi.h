/*
 * ncf_abi.h — C ABI of libncf_hip.so, the MI355X (gfx950) hot path of the NCF scoring forward.
 *
 * The reference (michaelbzms/DeepRecommendation) is 100 % Python on PyTorch; it has no FFI, no custom
 * operator and no native code.  The "interface each entry point replaces" is therefore the sequence of
 * ATen ops a reference forward() issues; each declaration below cites it as
 * src/neural_collaborative_filtering/<file>:<line> of the reference.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - return 0 (NCF_OK) or a negative ncf_status; never throw.  ncf_last_error() returns a thread-local
 *     human-readable message for the last failure on the calling thread.
 *   - every pointer named dev_* / documented "device" is a HIP device pointer owned by the caller; the
 *     library never allocates persistent device memory, never synchronises the stream, never copies to the
 *     host.  Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - index arrays are int64 at the ABI (the reference uses torch.long: datasets/gnn_datasets.py:28);
 *     CSR column ids are int32 (node counts < 2^31).
 *   - leading dimensions (ld*) are in ELEMENTS of the tensor's dtype.
 *   - re-entrant and thread-safe.  State held by the library, all of it listed here: the thread-local error
 *     string; the process-wide option table written only by ncf_set_option (atomic ints, every option defaults to
 *     0 = "choose by shape and size"; no entry point reads the environment); a per-device cache of the CU count;
 *     and the dynamic-LDS limit of the attention kernels, raised once per kernel instantiation and device.
 *   - out-of-range indices never fault: the offending row is read as zeros and, when `dev_oob_flag` is
 *     non-NULL, *dev_oob_flag is set to 1 (the host wrapper turns that into IndexError on request, which is
 *     what torch indexing raises in the reference).
 */
#ifndef NCF_ABI_H
#define NCF_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCF_ABI_VERSION 1

typedef void* ncf_stream_t; /* hipStream_t */

enum ncf_dtype { NCF_F32 = 0, NCF_BF16 = 1 };

enum ncf_status {
    NCF_OK = 0,
    NCF_EINVAL = -1,       /* bad argument (null pointer, negative size, misaligned, inconsistent dims) */
    NCF_EUNSUPPORTED = -2, /* shape/dtype has no specialised kernel: caller should take the unfused entry points */
    NCF_ELAUNCH = -3,      /* HIP reported an error at launch */
    NCF_EWORKSPACE = -4    /* workspace too small */
};

int ncf_version(void);
const char* ncf_last_error(void);
/* Architecture the device code was compiled for ("gfx950"). */
const char* ncf_build_arch(void);
/* Hash (16 hex digits) of the sources, headers and compiler flags this library was built from — csrc/build.py:source_id().  The
 * Python binding and __graft_entry__.build() refuse a library whose id differs from the sources next to it (a stale .so). */
const char* ncf_build_id(void);

/* Process-wide kernel-selection overrides for A/B measurements and for tests that must drive every kernel variant
 * (no counterpart upstream).  0 always means "choose by shape and size" (the default).  Options:
 *   "bf16_kernel"          1 = 4-wave weight-stationary kernel, 2 = slab-streaming kernel, 3 = 8-wave weight-stationary kernel
 *                          (ncf_score_fused, NCF_BF16; 3 falls back to 1 on shapes it does not take)
 *   "linear_kernel"        1 = one row tile per wave, 2 = persistent row-streaming form          (ncf_mlp_forward / ncf_linear_forward)
 *   "linear_kslices"       4 | 8 = K-slices of the skinny-deep Linear form
 *   "attn_grouped_kernel"  1 = LDS-broadcast form, 2 = scalar-operand form                       (ncf_attn_forward_grouped)
 *   "gather_kernel"        1 = one step per wave, 2 = persistent prefetching waves                (ncf_gather_concat)
 * Every variant of one entry computes the same function (bit-identical where the entry promises it).
 * NCF_EINVAL for an unknown name or a value outside the option's set. */
int ncf_set_option(const char* name, int value);
int ncf_get_option(const char* name, int* value);

/* ------------------------------------------------------------------------------------------------
 * K1  embedding gather (+ fused concat)
 * Replaces: nn.Linear applied to one-hot rows + torch.cat — models/basic_ncf.py:38-40, models/mf.py:29-30;
 *           combined_graph_emb[itemIds] / [userIds] + cat — models/gnn_ncf.py:354-361.
 * out[p, 0:EA] = tabA[idxA[p], 0:EA];  out[p, EA:EA+EB] = tabB[idxB[p], 0:EB]     (bit-exact copy)
 * tabB/idxB may be NULL with EB = 0 (single-table gather).  idxA / idxB may be NULL = identity (row p).
 * ------------------------------------------------------------------------------------------------ */
int ncf_gather_concat(int dtype,
                      const void* dev_tabA, int64_t rowsA, int64_t ldA,
                      const void* dev_tabB, int64_t rowsB, int64_t ldB,
                      const int64_t* dev_idxA, const int64_t* dev_idxB,
                      int64_t B, int EA, int EB,
                      void* dev_out, int64_t ldOut,
                      int32_t* dev_oob_flag, ncf_stream_t stream);

/* Row-wise dot product of two gathered rows, out[p] = sum_e tabA[idxA[p], e] * tabB[idxB[p], e]  (fp32
 * accumulate, fp32 out).  Replaces: torch.bmm(user_emb.unsqueeze(1), item_emb.unsqueeze(2)) —
 * models/mf.py:31, models/gnn_ncf.py:365. */
int ncf_gather_dot(int dtype,
                   const void* dev_tabA, int64_t rowsA, int64_t ldA,
                   const void* dev_tabB, int64_t rowsB, int64_t ldB,
                   const int64_t* dev_idxA, const int64_t* dev_idxB,
                   int64_t B, int E, float* dev_out,
                   int32_t* dev_oob_flag, ncf_stream_t stream);

/* Exchange preparation for ROW-SHARDED tables (BASELINE config 5: the table outgrows one GPU; the reference is single
 * device — its lookup is the nn.Linear on one-hot rows of models/basic_ncf.py:38-39 — so this has no upstream counterpart).
 * Rank o of `world` owns rows [o * rows_per_rank, (o+1) * rows_per_rank) of a table of total_rows rows.  Lists the batch's
 * ids by owner in a FIXED-capacity send buffer so that the all-to-all exchanges that follow use equal splits and need
 * no size on the host:
 *   dev_send[o * cap + k] = id - o * rows_per_rank   for the k-th id of owner o (k < cap; order inside a bucket unspecified);
 *                           unused slots are 0 (a valid local row wherever the shard is not empty)
 *   dev_slot[p]           = o * cap + k  — the row of pair p in the (world * cap)-row buffer the row exchange returns;
 *                           -1 for an id outside [0, total_rows) (sets *dev_oob_flag) or beyond its bucket's capacity
 *                           (sets *dev_overflow_flag): such a pair then reads as an out-of-range row downstream
 *   dev_counts[o]         = number of ids owned by o (may exceed cap)
 * dev_send (world * cap) and dev_counts (world) are zero-filled by this call.  world <= 1024. */
int ncf_bucket_ids(const int64_t* dev_idx, int64_t B, int64_t rows_per_rank, int64_t total_rows, int world, int64_t cap,
                   int64_t* dev_send, int64_t* dev_slot, int32_t* dev_counts,
                   int32_t* dev_oob_flag, int32_t* dev_overflow_flag, ncf_stream_t stream);

/* De-duplicating form of ncf_bucket_ids ("dedup duplicate ids per destination before sending"): every DISTINCT id
 * of the batch takes one slot of its owner's bucket and all of its pairs share it (dev_slot), through a hash set in device memory
 * — no sort, no size on the host.  Buckets carry their count: dev_send holds world buckets of (cap + 1) int64,
 * [count, id_0 .. id_{cap-1}], so the counts travel with the id all-to-all and the owner gathers count rows per bucket
 * (ncf_gather_buckets); padding is never initialised.  dev_slot[p] indexes the (world * cap) rows that come back.
 * dev_hkeys / dev_hvals: table_slots >= ncf_bucket_dedup_table_slots(B) int64 each (a power of two >= 2 B), caller-owned scratch.
 * Flags as ncf_bucket_ids.  The reference has no counterpart (single device). */
size_t ncf_bucket_dedup_table_slots(int64_t B);
int ncf_bucket_ids_dedup(const int64_t* dev_idx, int64_t B, int64_t rows_per_rank, int64_t total_rows, int world, int64_t cap,
                         int64_t* dev_hkeys, int64_t* dev_hvals, int64_t table_slots,
                         int64_t* dev_send, int64_t* dev_slot, int32_t* dev_counts,
                         int32_t* dev_oob_flag, int32_t* dev_overflow_flag, ncf_stream_t stream);

/* The owner's gather for the buckets of ncf_bucket_ids_dedup: dev_recv = world buckets of [count, ids ...] as received;
 * out row (r * cap + k) = table[recv[r][1 + k]] for k < count_r; rows beyond a bucket's count are neither read nor written.
 * Rows must be multiples of 16 bytes.  An id outside [0, rows) gives a zero row and sets *dev_oob_flag. */
int ncf_gather_buckets(int dtype, const void* dev_table, int64_t rows, int64_t ld, const int64_t* dev_recv, int world, int64_t cap, int E,
                       void* dev_out, int64_t ldout, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K2  MLP forward, generic layer-by-layer path (any dims)
 * Replaces: nn.Sequential(Linear, [ReLU, Dropout(eval = identity), Linear]*) — util.py:5-18, called at
 *           models/basic_ncf.py:41, models/attention_ncf.py:179,222, models/gnn_ncf.py:362; and single
 *           nn.Linear layers (n_layers = 1): models/attention_ncf.py:150-151,216, models/gnn_ncf.py:300-301,
 *           the hoisted per-node form of gnn_ncf.py:91-93.
 * dims[0] = input width, dims[i] = out_features of layer i (i = 1..n_layers).  W[i] is device [dims[i+1]][dims[i]]
 * row-major (torch nn.Linear.weight layout), b[i] is device [dims[i+1]] (may be NULL = no bias).
 * ReLU is applied between layers, never after the last one.  Intermediates live in `dev_workspace`
 * (ncf_mlp_workspace_bytes).  fp32 only on this entry (NCF_F32); accumulation is an exact fp32 FMA chain
 * (v_mfma_f32_32x32x2_f32).
 * `host_W` / `host_b` are HOST arrays of DEVICE pointers.
 * ------------------------------------------------------------------------------------------------ */
size_t ncf_mlp_workspace_bytes(int dtype, int64_t B, int n_layers, const int* dims);
int ncf_mlp_forward(int dtype, const void* dev_x, int64_t B, int64_t ldx,
                    int n_layers, const int* dims,
                    const void* const* host_W, const void* const* host_b,
                    void* dev_workspace, size_t workspace_bytes,
                    void* dev_out, int64_t ldOut, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K1+K2 fused: gather -> concat -> MLP -> (B,1) without the (B, EA+EB) round trip through HBM.
 * Replaces the whole of models/basic_ncf.py:37-42 (table form) and models/gnn_ncf.py:354-362.
 *
 * The MLP must end in a 1-wide layer (util.py:10 output_size = 1): dims = {EA+EB, h1, [h2,] 1}.
 * Weights are passed PRE-PACKED (ncf_mlp_pack) in the lane order the MFMA operands are consumed in, so a
 * wave streams them with fully coalesced 16-byte loads; pack once per model, reuse for every batch.
 * Returns NCF_EUNSUPPORTED when (dtype, EA, EB, dims) has no specialised instance — use
 * ncf_gather_concat + ncf_mlp_forward then.  ncf_score_fused_supported() answers without launching.
 * idxA / idxB NULL = identity, so a dense activation matrix x (B, K0) can be scored with tabA = x, EB = 0.
 * ------------------------------------------------------------------------------------------------ */
int ncf_score_fused_supported(int dtype, int EA, int EB, int n_layers, const int* dims);
size_t ncf_mlp_packed_bytes(int dtype, int n_layers, const int* dims);
int ncf_mlp_pack(int dtype, int n_layers, const int* dims,
                 const void* const* host_W, const void* const* host_b,
                 void* dev_packed, size_t packed_bytes, ncf_stream_t stream);
int ncf_score_fused(int dtype,
                    const void* dev_tabA, int64_t rowsA, int64_t ldA,
                    const void* dev_tabB, int64_t rowsB, int64_t ldB,
                    const int64_t* dev_idxA, const int64_t* dev_idxB,
                    int64_t B, int EA, int EB,
                    int n_layers, const int* dims, const void* dev_packed,
                    float* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);

/* Partial first layer (frozen weights), BIT-IDENTICAL to ncf_score_fused: layer 1's MFMA chain of every neuron starts from
 * b1 and runs over table A's EA/8 k-groups first, so after them it holds a value that depends on the row of A only.
 * ncf_layer1_partial writes that value for every row of A, plus row rowsA for an out-of-range id, as the fp32 table
 * P (rowsA + 1, N1), ldP >= N1, with the same MFMA instructions; build it once per weight version.
 * ncf_score_fused_partial then returns exactly what ncf_score_fused returns for the same arguments while issuing layer 1
 * over table B's groups only (3/4 of the MFMAs of a tile at 128-256-128-1).  Small batches and a ragged last round of
 * 4 x CUs tiles go to ncf_score_fused's own kernels, as there.  Out-of-range ids set *dev_oob_flag.
 * Supported (ncf_score_fused_partial_supported): dtype NCF_F32, EA > 0, EB in {32, 64, 96, 128}, and a shape that
 * ncf_score_fused supports; else NCF_EUNSUPPORTED.  ncf_score_fused_partial_in_lds answers 1 where the kernel of that shape
 * keeps table B's half of layer 1's weights in LDS (EB/8 * N1/32 KiB <= 80), 0 where it streams them or has no kernel. */
int ncf_score_fused_partial_supported(int dtype, int EA, int EB, int n_layers, const int* dims);
int ncf_score_fused_partial_in_lds(int dtype, int EA, int EB, int n_layers, const int* dims);
int ncf_layer1_partial(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, int EA, int EB,
                       int n_layers, const int* dims, const void* dev_packed,
                       void* dev_P, int64_t ldP, ncf_stream_t stream);
int ncf_score_fused_partial(int dtype, const void* dev_P, int64_t ldP,
                            const void* dev_tabA, int64_t rowsA, int64_t ldA,
                            const void* dev_tabB, int64_t rowsB, int64_t ldB,
                            const int64_t* dev_idxA, const int64_t* dev_idxB,
                            int64_t B, int EA, int EB,
                            int n_layers, const int* dims, const void* dev_packed,
                            float* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);

/* Opt-in inference-time folding of the first MLP layer into the tables (frozen weights):
 *   relu(W1 . cat(a, b) + b1) == relu(PA[ia] + PB[ib])  with  PA = TA . W1[:, :EA]^T + b1  (rowsA, N1)  and
 *   PB = TB . W1[:, EA:]^T  (rowsB, N1), both built once by the caller (ncf_mlp_forward with n_layers = 1).
 * out[p] = tail( relu(PA[idxA[p]] + PB[idxB[p]]) ),  tail = the remaining MLP [N1 -> N2 -> 1] packed by
 * ncf_mlp_pack(dims = {N1, N2, 1}).  Same function as ncf_score_fused up to fp32 summation order; layer 1 costs no
 * matrix work, the gathered rows are N1 wide (4x the bytes at E = 64, N1 = 256).  Replaces basic_ncf.py:38-41 /
 * gnn_ncf.py:354-362 like ncf_score_fused.  NCF_EUNSUPPORTED when (N1, N2) has no instance. */
int ncf_score_folded_supported(int dtype, int N1, int N2);
int ncf_score_folded(int dtype,
                     const void* dev_PA, int64_t rowsA, int64_t ldPA,
                     const void* dev_PB, int64_t rowsB, int64_t ldPB,
                     const int64_t* dev_idxA, const int64_t* dev_idxB,
                     int64_t B, int N1, int N2, const void* dev_packed_tail,
                     float* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K4/K5  LightGCN propagation as CSR-by-destination SpMM with a wavefront segmented reduction
 * Replaces: PyG MessagePassing.propagate(aggr='add') + message() — models/gnn_ncf.py:52-70,74-94
 *           (per-edge Linear hoisted to a per-node Linear, which is ncf_mlp_forward with n_layers = 1),
 *           torch_geometric.utils.degree + deg.pow(-0.5) — gnn_ncf.py:47-50,
 *           torch.mean(torch.stack(hs)) — gnn_ncf.py:351 (running sum fused into the SpMM epilogue).
 *
 * Segment s owns edges [segptr[s], segptr[s+1]) and belongs to destination row row_of[s] (row_of == NULL:
 * row s, i.e. segptr is a plain CSR rowptr).  Long rows may be split by the caller into several CONSECUTIVE
 * segments (load balance under Zipf-skewed degrees); their partial sums are added in segment order, so
 *   y[n, :] = sum over the segments of row n, in order, of  sum_{e in segment} coef[e] * z[col[e], :]
 * is bitwise reproducible (no float atomics).  Every row must own at least one (possibly empty) segment.
 * if dev_sum != NULL:  dev_sum[n, :] += y[n, :]   (layer-sum accumulator for the final mean)
 * z is (Nz, D) with leading dimension ldz; y and sum are (N, D).  D % 4 == 0, D <= 256.
 * coef may be NULL (all ones).  dev_partial: (n_seg, D) floats scratch, required when dev_row_of != NULL.
 * fixup = 1: rows split over several segments are completed inside this call (one lane group per row walks its
 *   partials in order — simple, but serial per row).
 * fixup = 0: such rows are NOT written; their per-segment sums stay in dev_partial[s, :] and the caller finishes them
 *   with further calls of this same entry (z = dev_partial, col = segment ids, coef = NULL, segments of the partial
 *   list) until every row is down to one segment — a log-depth ordered tree, used for hub rows with millions of edges.
 * ------------------------------------------------------------------------------------------------ */
int ncf_spmm_csr(int dtype, const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg,
                 const int32_t* dev_col, const float* dev_coef,
                 const void* dev_z, int64_t Nz, int64_t ldz, int D,
                 void* dev_y, int64_t ldy, float* dev_sum, int64_t ldsum,
                 float* dev_partial, int fixup, ncf_stream_t stream);

/* Training-step form of ncf_spmm_csr: the reference applies Dropout INSIDE the per-edge Linear of a LightGCN layer
 * (gnn_ncf.py:22-31, 91-93: message_e = coef_e * dropout_p(W(x[src_e])), one mask element per (edge, feature), kept values
 * scaled by 1 / (1 - p)), which a per-node hoisted Linear cannot express.  Here the mask is regenerated inside the kernel from a
 * counter-based hash of (seed, edge id, feature): element (e, f) of the mask is a pure function of the three, so
 *   forward   y  = sum_e coef_e * mask(id_e, :) / (1 - p') * z[col_e]        (CSR by destination, dev_edge_id = NULL: id = position)
 *   backward  dz = the same call on the CSR by SOURCE with dev_edge_id[.] = each entry's position in the forward CSR
 * use the same mask without storing it.  The masks are NOT torch's Philox stream: a seeded run differs from the reference's in
 * the (random) masks drawn, not in their law.  Only edge-level calls take a mask (the partial-sum tree levels of split rows go
 * through ncf_spmm_csr).
 *
 * THE MASK (part of this ABI, shared with ncf_attn_forward_dropout / ncf_attn_backward; restated in numpy by
 * tests/dropout_mask_ref.py, which the kernels are held to element by element).  For entry e, taken modulo 2^32, and 16-byte
 * chunk c (features 4c .. 4c+3), in uint32 arithmetic:
 *       h0 = lowbias32(e * 0x9E3779B1 ^ seed ^ c * 0x85EBCA77)
 *       h1 = lowbias32(h0 ^ 0x68E31DA4)
 *   with lowbias32 as under ncf_sample_negatives below.  Features 4c, 4c+1, 4c+2, 4c+3 are KEPT iff
 *       h0 & 0xFFFF,  h0 >> 16,  h1 & 0xFFFF,  h1 >> 16      respectively are >= thr,
 *       thr = (uint32)(p * 65536.f + 0.5f)   evaluated in fp32 (halves round up), clamped to 65535,
 *   so the drop probability is p' = thr / 65536.  Kept values are multiplied by the fp32 quotient 65536.f / (float)(65536 - thr)
 *   (= 1 / (1 - p') rounded to fp32, NOT 1 / (1 - p)); dropped ones are 0.  thr = 0 (p < 2^-17, p = 0 included) takes the plain
 *   kernel: the result is ncf_spmm_csr's bit for bit.  p outside [0, 1) or NaN: NCF_EINVAL.
 *   e here: entry k of the call's CSR has e = dev_edge_id[k] when dev_edge_id is given, else e = k, its position in dev_col
 *   (for the forward call that is the position in the CSR by destination, whatever segment or tree level handles it). */
int ncf_spmm_csr_dropout(int dtype, const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg,
                         const int32_t* dev_col, const float* dev_coef,
                         const void* dev_z, int64_t Nz, int64_t ldz, int D,
                         void* dev_y, int64_t ldy, float* dev_sum, int64_t ldsum,
                         float* dev_partial, int fixup, const int32_t* dev_edge_id, uint32_t seed, float p, ncf_stream_t stream);

/* deg[n] = number of edges whose destination is n (float, exact below 2^24) — PyG degree(), gnn_ncf.py:48.
 * dev_deg must be zero-filled by the caller; two calls (u2i, i2u) accumulate into the same array, which is
 * the cat at gnn_ncf.py:41. */
int ncf_degree_accumulate(const int64_t* dev_dst, int64_t E, int64_t N, float* dev_deg,
                          int32_t* dev_oob_flag, ncf_stream_t stream);
/* coef[e] = (attr ? attr[e] : 1) * (dis[src[e]] * dis[dst[e]]),  dis = deg^-1/2 with inf -> 0
 * (gnn_ncf.py:49-50,54,58,66 and the product order of :91 / :93). */
int ncf_edge_coef(const int64_t* dev_src, const int64_t* dev_dst, const float* dev_attr,
                  const float* dev_deg, int64_t E, int64_t N, float* dev_coef, ncf_stream_t stream);

/* Which edges one GraphNCF training step keeps (gnn_ncf.py:246-296, 314-320): the batch's target edges, node dropout and message
 * dropout only choose the edges that take part in a step.  The CSR never changes: a removed edge is an edge of weight 0, and the
 * degrees are those of the remaining edges.  One pass over the level-0 segments of the CSR by destination (dev_segptr / dev_row_of
 * of ncf_spmm_csr, one wave per segment; dev_row_of == NULL: segment s is row s).  For entry e with source dev_col[e] and
 * destination = its segment's row:
 *     kept      = dev_pair_key[e] is not among dev_targets_sorted[0 .. n_targets)              (n_targets = 0: no target masking)
 *                 AND dev_node_keep[src] & dev_node_keep[dst]                                   (dev_node_keep = NULL: no node dropout)
 *                 AND the message rule below on dev_slot[e]                                     (thr = 0: dev_slot may be NULL)
 *     w_out[e]  = kept ? (dev_attr ? dev_attr[e] : 1.f) : 0.f
 *     deg_out[row] = number of kept entries of the row       (cleared by this call; each segment adds its count with one integer
 *                    atomic add — integer sums do not depend on arrival order, so the result is bitwise reproducible)
 * dev_targets_sorted: the batch's user * N + item keys in ascending order, duplicates allowed (a per-lane binary search).
 * dev_pair_key[e]: the same key of entry e's edge, whichever direction it runs.  A source outside [0, N) counts as not kept when
 * dev_node_keep is given.  w_out then goes into ncf_edge_coef as attr with deg_out (as floats) as deg: a row left with no edge
 * has dis = 0 there, so all its coefficients are 0.
 *
 * THE KEEP RULE (part of this ABI; restated in numpy by tests/edge_keep_ref.py, which the kernel is held to bit for bit).
 *   Message dropout (gnn_ncf.py:246-279: an edge is kept with probability 1 - p, nothing is rescaled).  In uint32 arithmetic:
 *       thr = (uint32)(p * 65536.f + 0.5f)   evaluated in fp32, clamped to 65535          (as in THE MASK above)
 *       h   = lowbias32((uint32)slot * 0x9E3779B1 ^ (uint32)seed)                          (lowbias32: under ncf_sample_negatives)
 *       kept iff (h >> 16) >= thr
 *     slot of edge j of user2item_edge_index is j.  slot of edge j of item2user_edge_index is also j when both lists have the
 *     same length and both edge attributes are present (the reference's "symmetrical" branch :254-264: one mask bit removes both
 *     directions), else E1 + j with E1 the length of user2item_edge_index (independent masks, :266-277).  The condition is
 *     evaluated on the graph's own lists, not on the lists after target masking.
 *   Node dropout (gnn_ncf.py:281-296: subgraph over the kept nodes).  Every node of the batch is kept; of the other nodes exactly
 *     K = int((1.0 - p) * (N - nb)) (float64) are kept, nb = number of distinct batch nodes: the K smallest by (key(n), n) with
 *       key(n) = lowbias32((uint32)n * 0x9E3779B1 ^ (uint32)node_seed).
 *     The caller builds the byte mask dev_node_keep (N) from this rule; an edge survives iff both its ends are kept.
 * p outside [0, 1] or not finite, negative sizes, a null required pointer (dev_slot with thr > 0 included): NCF_EINVAL, and
 * nothing is launched. */
int ncf_edge_keep(const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg, int64_t N,
                  const int32_t* dev_col, const float* dev_attr,
                  const int64_t* dev_pair_key, const int64_t* dev_targets_sorted, int64_t n_targets,
                  const int32_t* dev_slot, float p, uint32_t seed,
                  const uint8_t* dev_node_keep,
                  float* dev_w_out, int32_t* dev_deg_out, ncf_stream_t stream);
/* LightGAT edge attention over a CSR-by-destination graph (models/gnn_ncf.py:151-177; PyG softmax(src, index) =
 * exp(src - max_group) / (sum_group + 1e-16)):
 *   dev_out[e] = (attr ? attr[e] : 1) * softmax over the edges of e's destination row of s[col[.]]
 * s[n] = w_j . x[n] is the source half of AttNet(cat(x_j, x_i)) (the destination half + bias is constant inside a
 * group and cancels in the softmax).  The result is the per-edge coefficient for ncf_spmm_csr. */
int ncf_edge_softmax_csr(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_attr, const float* dev_s,
                         int64_t n_rows, int64_t Ns, float* dev_out, ncf_stream_t stream);
/* The same function over the SEGMENTS of the SpMM's split rows (dev_segptr / dev_row_of of ncf_spmm_csr, dev_seg_first[r] = first
 * segment of row r, n_rows + 1 entries): three passes parallel over segments / rows instead of one wave per destination — a hub
 * destination with millions of in-edges no longer serialises.  Fixed order, no atomics; equal to ncf_edge_softmax_csr up to the
 * fp32 summation order.  workspace: ncf_edge_softmax_segmented_workspace_bytes(n_seg, n_rows). */
size_t ncf_edge_softmax_segmented_workspace_bytes(int64_t n_seg, int64_t n_rows);
int ncf_edge_softmax_segmented(const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg, const int64_t* dev_seg_first,
                               int64_t n_rows, const int32_t* dev_col, const float* dev_attr, const float* dev_s, int64_t n_src,
                               float* dev_out, void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);

/* LightGAT TRAINING STEP (models/gnn_ncf.py:151-177 with autograd recording).  z = W(x) is hoisted per node as for LightGCN and
 * s[n] = w_j . x[n] is the source half of AttNet (the destination half and the bias are constant in a softmax group and cancel).
 * For destination row r with KEPT entries e (kept = dev_keep[e] != 0 and dev_col[e] in range; dev_keep = NULL: all kept):
 *     alpha_e = exp(s[col_e] - M_r) / (sum_kept exp(s[col_.] - M_r) + 1e-16)      M_r = max over the kept entries of the row
 *     coef_e  = (attr ? attr_e : 1) * alpha_e
 *     y[r]    = sum_e coef_e * drop_e(z[col_e])                                    ncf_spmm_csr_dropout (THE MASK, e = CSR position)
 * and backward for a given dY:
 *     dZ[n]    = sum_{e: col_e = n} coef_e * drop_e(dY[row_e])                     ncf_spmm_csr_dropout on the CSR by source
 *     g_e      = (attr ? attr_e : 1) * < dY[row_e], drop_e(z[col_e]) >
 *     S_r      = sum_{e in r} alpha_e * g_e
 *     dlogit_e = alpha_e * (g_e - S_r)              exact also with the 1e-16: d alpha_e / d t_k = delta alpha_e - alpha_e alpha_k
 *     ds[n]    = sum_{e: col_e = n} dlogit_e
 * A removed entry and an entry whose col is out of range are not in their group: alpha = coef = dlogit = 0.  A row with no kept
 * entry produces 0 everywhere; nothing is NaN or inf for finite inputs.
 * All three entries walk the level-0 segments of the prepared CSR (dev_segptr / dev_row_of of ncf_spmm_csr, dev_seg_first[r] =
 * first segment of row r, n_rows + 1 entries; dev_row_of == NULL: segment s is row s, n_seg == n_rows, dev_seg_first unused).
 * Loops are bounded by the segment ends only.  No float atomics, a fixed summation order: every output is bitwise repeatable.
 * A null required pointer, a negative size, D % 4 != 0, p outside [0, 1) or not finite: NCF_EINVAL; D > 256: NCF_EUNSUPPORTED; a
 * short workspace: NCF_EWORKSPACE — and nothing is launched.
 *
 * ncf_gat_edge_softmax: dev_alpha_out[E], and dev_coef_out[E] when dev_attr is given.  The three passes and the operation order of
 * ncf_edge_softmax_csr (dev_row_of == NULL) / ncf_edge_softmax_segmented: with dev_keep == NULL, alpha * attr is their dev_out
 * bit for bit.  dev_keep is the dev_w_out of ncf_edge_keep called with dev_attr = NULL (exactly 1 / 0), so a kept edge whose
 * weight is 0 still counts in its group.  The workspace is needed only with dev_row_of. */
size_t ncf_gat_edge_softmax_workspace_bytes(int64_t n_seg, int64_t n_rows);
int ncf_gat_edge_softmax(const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg, const int64_t* dev_seg_first,
                         int64_t n_rows, const int32_t* dev_col, const float* dev_attr, const float* dev_keep, const float* dev_s,
                         int64_t n_src, float* dev_alpha_out, float* dev_coef_out, void* dev_workspace, size_t workspace_bytes,
                         ncf_stream_t stream);
/* ncf_gat_edge_grad: dev_dlogit_out[E] from dY (n_rows, D), z (Nz, D) (hoisted, before dropout), alpha of ncf_gat_edge_softmax and
 * the forward's (p, seed).  One wave per segment in the lane layout of ncf_spmm_csr (D % 4 == 0, D <= 256, rows 16-byte aligned);
 * rows split over segments get S_r in a per-row pass over the segment sums.  An entry with alpha == 0 reads no z row. */
size_t ncf_gat_edge_grad_workspace_bytes(int64_t n_seg, int64_t n_rows);
int ncf_gat_edge_grad(const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg, const int64_t* dev_seg_first, int64_t n_rows,
                      const int32_t* dev_col, const float* dev_attr, const float* dev_alpha, const float* dev_dY, int64_t ldy,
                      const float* dev_z, int64_t Nz, int64_t ldz, int D, float p, uint32_t seed, float* dev_dlogit_out,
                      void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);
/* ncf_gat_source_reduce: ONE LEVEL of ds[n] = sum_k dev_val[dev_idx[k]] over row n of the CSR by source (dev_idx = the transpose's
 * edge ids; NULL: k itself; ids outside [0, n_val) are skipped).  The segment walk of ncf_spmm_csr on scalars: a segment that is
 * the first and the last of its row writes dev_out[row] (0 for an empty row), any other writes its sum to dev_partial[segment]
 * (when given); the caller re-applies the entry to the partial sums level by level, as for ncf_spmm_csr's split rows. */
int ncf_gat_source_reduce(const int64_t* dev_segptr, const int32_t* dev_row_of, int64_t n_seg, const int32_t* dev_idx,
                          const float* dev_val, int64_t n_val, float* dev_out, int64_t n_rows, float* dev_partial,
                          ncf_stream_t stream);

/* out[n, :] = in[n, :] / divisor (the division of torch.mean over the L+1 stacked layers, gnn_ncf.py:351). */
int ncf_scale_rows(const float* dev_in, int64_t ldin, int64_t N, int D, float divisor,
                   float* dev_out, int64_t ldout, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K3  AttentionNCF item-item attention: scores -> masked row softmax -> rating-weighted aggregation
 * Replaces models/attention_ncf.py:154-213 (eval mode).  Inputs are the *projected* operands:
 *   att_dense > 0 (AttentionNet = Linear(2·IE -> A), ReLU, Linear(A -> 1), :112-117):
 *       dev_pc (B, A)   = cand_emb  @ W0[:, :IE]^T + b0        (candidate half of AttentionNet.0, bias folded)
 *       dev_pr (I, A)   = rated_emb @ W0[:, IE:]^T            (rated half)
 *       score(b, i)     = b1 + sum_a w1[a] * relu(pc[b, a] + pr[i, a])
 *     which is AttentionNet(cat(cand, rated)) with the first Linear split at the concat boundary (:176).
 *   att_dense == 0 (AttentionNet = Linear(2·IE -> 1), :120-122): A = 1, no ReLU:
 *       score(b, i) = pc[b, 0] + pr[i, 0]
 *   cosine (:162-173): dev_pc / dev_pr are the L2-normalised embeddings (B, IE) / (I, IE), mode = NCF_ATT_COS,
 *       score = dot.
 * The user's rated set is CSR: row b owns entries [rowptr[b], rowptr[b+1]) with col = position in the rated
 * list (0..I-1) and val = the non-zero user_matrix entry (:158 `user_matrix != 0`).
 *   w = softmax over the row's entries (empty row -> all zeros, :208-209)
 *   dev_out_feat[b, :] = bias + sum_i  w[b,i] * val[b,i] * feat[col_i, :]      (:212-213), feat is (I, Fdim)
 *     feat may be the raw item features (Fdim = F; bias NULL; UserEmbeddings applied afterwards, :216) or, using
 *     the linearity of UserEmbeddings over the weighted sum, the pre-projected rows feat = rated_items @ Wu^T
 *     (Fdim = UE) with dev_out_bias = bu — then dev_out_feat IS user_embeddings of :216.
 *   dev_weights ((nnz,) floats aligned with the CSR entries, REQUIRED: it doubles as the score scratch) receives
 *     the attention weights w (what return_attention_weights exposes, :224).
 * ------------------------------------------------------------------------------------------------ */
/* NCF_ATT_MLP_SCALED: NCF_ATT_MLP whose caller pre-multiplied dev_pc and dev_pr by 2^-NCF_ATT_SCALE_LOG2 and dev_w1 by
 * 2^NCF_ATT_SCALE_LOG2 (fold the factors into the weights that produce them: exact, powers of two).  The function is
 * unchanged bit for bit — w' relu(p' + q') == w relu(p + q) — but in scaled units every sum lies in (-1, 1), so the
 * grouped kernel may evaluate relu as the [0, 1] CLAMP output modifier of its packed add (gfx950 has no packed fp32 max):
 * half the vector instructions of the score loop.  Differs from relu only where |pc + pr| >= 2^64 in true units (scores
 * that are numerically meaningless in fp32 anyway: they saturate instead of overflowing); a NaN sum gives 0 as with max. */
enum ncf_att_mode { NCF_ATT_MLP = 0, NCF_ATT_LINEAR = 1, NCF_ATT_COS = 2, NCF_ATT_MLP_SCALED = 3 };
#define NCF_ATT_SCALE_LOG2 64
int ncf_attn_forward(int mode,
                     const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A,
                     const float* dev_w1, float b1,
                     const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val,
                     int64_t B, int64_t I,
                     const float* dev_feat, int64_t ldfeat, int Fdim,
                     const float* dev_out_bias,
                     float* dev_out_feat, int64_t ldout,
                     float* dev_weights,
                     ncf_stream_t stream);

/* Training-step forms of ncf_attn_forward (the reference differentiates attention_ncf.py:176-216 through autograd):
 *   ncf_attn_forward_dropout  NCF_ATT_MLP with AttentionNet's hidden Dropout(p) active (attention_ncf.py:112-117: one mask element
 *       per (pair, rated entry, hidden unit), kept values scaled by 1 / (1 - p')): the mask is regenerated in the kernel from a
 *       counter-based hash of (seed, CSR entry, unit) — NOT torch's Philox stream, same law.  The mask, thr, p' and the fp32
 *       scale are exactly those written out under ncf_spmm_csr_dropout (THE MASK), with e = the entry's position in the per-pair
 *       CSR passed to the call (index into dev_col / dev_val / dev_weights, not the position inside its row) and chunk c = hidden
 *       units 4c .. 4c+3; the score is s_e = b1 + sum_a w1[a] * relu(pc[b,a] + pr[col_e,a]) * scale * keep(e, a).  thr = 0 runs the
 *       plain kernels (bit for bit ncf_attn_forward / the p = 0 backward).  With thr > 0 the call needs NCF_ATT_MLP or
 *       NCF_ATT_MLP_SCALED (the same kernel: the exact power-of-two operand scales commute with the mask), A % 4 == 0, A <= 256
 *       and ldpc, ldpr % 4 == 0; anything else (cosine, linear) is NCF_EUNSUPPORTED and launches nothing.
 *   ncf_attn_backward         gradients of ncf_attn_forward[_dropout] given dev_weights (the attention weights the forward wrote)
 *       and dev_dout (B, Fdim) = d loss / d dev_out_feat:
 *         dev_d_pc (B, A)            written
 *         dev_d_pr (I, A)            ADDED to (float atomics): zero it first          dev_d_feat (I, Fdim)  likewise
 *         dev_d_w1_part (B, A)       per-pair partial rows of d w1 (NCF_ATT_MLP; column-sum them with ncf_colsum)
 *       d b1 is exactly 0 (a shift of all scores cancels in the softmax); d out_bias = column sums of dev_dout (ncf_colsum).
 *       dev_scratch: nnz floats.  seed / p as in the forward call (p = 0: no dropout).  NCF_ATT_MLP(_SCALED) and NCF_ATT_COS;
 *       A, Fdim % 4 == 0 and <= 256. */
int ncf_attn_forward_dropout(int mode,
                             const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A,
                             const float* dev_w1, float b1,
                             const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val,
                             int64_t B, int64_t I,
                             const float* dev_feat, int64_t ldfeat, int Fdim, const float* dev_out_bias,
                             float* dev_out_feat, int64_t ldout, float* dev_weights,
                             uint32_t seed, float p, ncf_stream_t stream);
int ncf_attn_backward(int mode,
                      const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A, const float* dev_w1,
                      const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t B, int64_t I,
                      const float* dev_feat, int64_t ldfeat, int Fdim,
                      const float* dev_weights, const float* dev_dout, int64_t lddout,
                      float* dev_d_pc, int64_t ldd_pc, float* dev_d_pr, int64_t ldd_pr, float* dev_d_w1_part,
                      float* dev_d_feat, int64_t ldd_feat, float* dev_scratch,
                      uint32_t seed, float p, ncf_stream_t stream);

/* The training pair with AttentionNCF's MESSAGE dropout (attention_ncf.py:184-189: F.dropout over the (pair, rated entry) logits, then
 * `attOut[attOut == 0] = -inf` before the softmax).  Arguments as ncf_attn_forward_dropout / ncf_attn_backward, then the message
 * dropout's own.  With thr_m, p' and the fp32 scale_m computed from msg_p exactly as thr, p' and the scale under THE MASK:
 *   forward   raw_e  = the score of ncf_attn_forward_dropout (b1 and the hidden mask under `seed` included; the dot product for cosine)
 *             keep_e = element (entry e, feature 0) of THE MASK under msg_seed: lowbias32(e * 0x9E3779B1 ^ msg_seed) & 0xFFFF >= thr_m,
 *                      e = the entry's position in the per-pair CSR of the call, as for the hidden mask
 *             s_e    = keep_e ? raw_e * scale_m : 0      (one fp32 product)
 *             s_e == 0 (either sign) becomes -inf: a dropped entry leaves the softmax, and so does a KEPT entry whose score is exactly
 *             zero — the reference's test cannot tell the two apart.  Softmax and aggregation are ncf_attn_forward's; a row whose
 *             entries are all dropped has zero weights and dev_out_feat = bias.
 *   backward  a dropped entry has weight 0, so its ds_e, its share of d feat and its score gradient are 0 already; for a kept entry the
 *             logit is scale_m * raw_e, so the only change is ds_e = scale_m * w_e (dpv_e - t).  No mask is regenerated and no message
 *             seed is taken.  d b1 stays exactly 0: scale_m * b1 is one shift over the kept entries, which cancels in the softmax.
 * thr_m = 0 (msg_p < 2^-17) runs the instantiations of ncf_attn_forward[_dropout] / ncf_attn_backward bit for bit; the zero rule is NOT
 * applied there (a message_dropout of 0 never applied it on this path).  msg_seed should differ from seed: with equal seeds the
 * entry's keep bit is hidden unit 0's.  NCF_ATT_MLP, NCF_ATT_MLP_SCALED and NCF_ATT_COS (hidden p must quantise to 0 for cosine);
 * NCF_ATT_LINEAR, or A, Fdim or a leading dimension outside ncf_attn_backward's conditions (multiples of 4, A, Fdim <= 256), is
 * NCF_EUNSUPPORTED and launches nothing, whatever msg_p.  p or msg_p outside [0, 1) or NaN: NCF_EINVAL. */
int ncf_attn_forward_train(int mode,
                           const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A,
                           const float* dev_w1, float b1,
                           const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val,
                           int64_t B, int64_t I,
                           const float* dev_feat, int64_t ldfeat, int Fdim, const float* dev_out_bias,
                           float* dev_out_feat, int64_t ldout, float* dev_weights,
                           uint32_t seed, float p, uint32_t msg_seed, float msg_p, ncf_stream_t stream);
int ncf_attn_backward_train(int mode,
                            const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A, const float* dev_w1,
                            const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t B, int64_t I,
                            const float* dev_feat, int64_t ldfeat, int Fdim,
                            const float* dev_weights, const float* dev_dout, int64_t lddout,
                            float* dev_d_pc, int64_t ldd_pc, float* dev_d_pr, int64_t ldd_pr, float* dev_d_w1_part,
                            float* dev_d_feat, int64_t ldd_feat, float* dev_scratch,
                            uint32_t seed, float p, float msg_p, ncf_stream_t stream);

/* The same computation for batches in which several pairs share one rated set (evaluation batches grouped by user;
 * serving one user against the whole catalogue, reference webapp/backend.py:78-121), LDS-tiled: the CSR has one row
 * per USER (n_rows rows), the B pairs are listed user by user —
 *   dev_grp_ptr (n_rows+1):  pairs of row r are dev_pair_ids[grp_ptr[r] .. grp_ptr[r+1])  (indices into pc / out rows)
 *   dev_wg_ptr  (n_rows+1):  exclusive prefix sum of ceil(pairs_of_row / pairs_per_wg)     (workgroups per row)
 * — and a workgroup stages a user's rated rows once per 64 entries into LDS for up to pairs_per_wg (1..32) pairs, with
 * an online softmax over the tiles.  Same result as ncf_attn_forward on the expanded per-pair CSR up to fp32 summation
 * order.  dev_weights (optional) receives the attention weights (models/attention_ncf.py:224) in the layout of that
 * expanded CSR: pair b's weights start at dev_weights[dev_weights_off[b]] and follow its row's entries
 * (dev_weights_off (B,) = exclusive prefix sum of the row lengths of pair_row[b]).
 * Fdim % 4 == 0 and ldfeat % 4 == 0 take the scalar-operand form (256-thread workgroups for pairs_per_wg <= 16, 512 threads for
 * 17..32: pc rows and w1 as scalar operands through the scalar cache, tiles by LDS-DMA, aggregation on the matrix cores); other
 * shapes the first, LDS-broadcast form.  ncf_attn_grouped_plan names the instantiation a shape runs.
 * NCF_EUNSUPPORTED (fall back to ncf_attn_forward): mode NCF_ATT_LINEAR, A % 4 != 0, A > 256, Fdim > 256. */
int ncf_attn_forward_grouped(int mode,
                             const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A,
                             const float* dev_w1, float b1,
                             const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val,
                             int64_t n_rows, int64_t n_rated,
                             const int64_t* dev_grp_ptr, const int64_t* dev_pair_ids, const int64_t* dev_wg_ptr,
                             int64_t B, int pairs_per_wg,
                             const float* dev_feat, int64_t ldfeat, int Fdim, const float* dev_out_bias,
                             float* dev_out_feat, int64_t ldout,
                             float* dev_weights, const int64_t* dev_weights_off, ncf_stream_t stream);

/* Which kernel ncf_attn_forward_grouped runs for a shape under the current "attn_grouped_kernel" option: the launch rule itself,
 * answered without launching and without touching the device (like ncf_linear_plan).  Any output pointer may be NULL.
 *   *form         0 nothing (B = 0 or n_rows = 0), 1 scalar-operand form (attn_grouped_sc_kernel<MODE, CPB, NW>), 2 LDS-broadcast
 *                 form (attn_grouped_kernel<MODE, FO, NPF>)
 *   *kernel_mode  the kernel's MODE: 0 MLP, 2 cosine, 3 MLP on the 2^-64-scaled operands with relu as a clamp (form 1 only; form 2
 *                 runs NCF_ATT_MLP_SCALED as MODE 0)
 *   *cpb_or_fo    form 1: CPB, the 16-byte chunks of a projected row per block of the score loop (32, 16, 8 or 1);
 *                 form 2: FO, the output registers per lane (1, 2 or 4 = ceil(Fdim / 64) rounded up)
 *   *nw_or_npf    form 1: NW, waves per workgroup (4 for pairs_per_wg <= 16, else 8); form 2: NPF, tile pieces per thread (4, 8, 16)
 *   *lds_bytes    dynamic LDS of the launch (above 64 KiB the entry raises the kernel's limit first)
 *   *grid_x       gridDim.x = ceil(B / pairs_per_wg) + min(n_rows, B), the bound on the number of groups
 * Status as ncf_attn_forward_grouped's for the same shape: NCF_EINVAL for bad sizes, ldfeat < Fdim or pairs_per_wg outside 1..32;
 * NCF_EUNSUPPORTED for NCF_ATT_LINEAR, A % 4 != 0, A > 256, Fdim > 256, a tile beyond 160 KiB of LDS, or the scalar-operand form
 * forced on a shape it does not take (Fdim % 4 != 0 or ldfeat % 4 != 0). */
int ncf_attn_grouped_plan(int mode, int A, int Fdim, int64_t ldfeat, int pairs_per_wg, int64_t B, int64_t n_rows,
                          int* form, int* kernel_mode, int* cpb_or_fo, int* nw_or_npf, int64_t* lds_bytes, int64_t* grid_x);

/* Builds dev_grp_ptr / dev_pair_ids / dev_wg_ptr of ncf_attn_forward_grouped from dev_pair_row (B,) = the CSR row of
 * each pair (what the dense user_matrix expresses by repeating a user's row, dynamic_datasets.py:24-40): a counting
 * sort on the stream, no host synchronisation.  The order of a row's pairs inside dev_pair_ids is unspecified (each
 * pair's output is independent of it).  A pair_row outside [0, n_rows) sets *dev_oob_flag (sticky) and drops the pair.
 * workspace: ncf_group_pairs_workspace_bytes(n_rows) bytes of device memory. */
size_t ncf_group_pairs_workspace_bytes(int64_t n_rows);
int ncf_group_pairs(const int64_t* dev_pair_row, int64_t B, int64_t n_rows, int pairs_per_wg,
                    int64_t* dev_grp_ptr, int64_t* dev_pair_ids, int64_t* dev_wg_ptr,
                    void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ncf_group_pairs that also writes dev_wg_row[w] = CSR row of workgroup w (int32, ceil(B / pairs_per_wg) + min(n_rows, B) slots —
 * the grid bound of the grouped kernels): ncf_attn_forward_split reads it instead of searching dev_wg_ptr. */
int ncf_group_pairs_rows(const int64_t* dev_pair_row, int64_t B, int64_t n_rows, int pairs_per_wg,
                         int64_t* dev_grp_ptr, int64_t* dev_pair_ids, int64_t* dev_wg_ptr, int32_t* dev_wg_row,
                         void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* Entry-split form of ncf_attn_forward_grouped (same operands and result; attention weights are not available here):
 * the rated set of a row is cut into `nsplit` slices of whole 64-entry tiles, one workgroup per (group of pairs, slice)
 * leaves a softmax partial (running maximum, sum, un-normalised aggregate) in dev_workspace and a second kernel of the same
 * call merges them in slice order (deterministic; merge = 0 leaves them for ncf_attn_tail).  Replaces the same reference lines as ncf_attn_forward_grouped
 * (models/attention_ncf.py:154-216); it exists because a batch of a few thousand pairs is too few workgroups of too long
 * a chain for the one-workgroup-per-group form.  nsplit = 1 needs no workspace and launches one kernel.
 * Shapes: ncf_attn_split_supported() (A % 32 == 0, A <= 256, Fdim 64 or 128, MLP / cosine modes); else NCF_EUNSUPPORTED.
 * dev_wg_row may be NULL (binary search over dev_wg_ptr). */
int ncf_attn_split_supported(int mode, int A, int Fdim, int pairs_per_wg);
size_t ncf_attn_split_workspace_bytes(int64_t B, int Fdim, int nsplit);
int ncf_attn_forward_split(int mode,
                           const float* dev_pc, int64_t ldpc, const float* dev_pr, int64_t ldpr, int A,
                           const float* dev_w1, float b1,
                           const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val,
                           int64_t n_rows, int64_t n_rated,
                           const int64_t* dev_grp_ptr, const int64_t* dev_pair_ids, const int64_t* dev_wg_ptr,
                           const int32_t* dev_wg_row, int64_t B, int pairs_per_wg,
                           const float* dev_feat, int64_t ldfeat, int Fdim, const float* dev_out_bias,
                           float* dev_out_feat, int64_t ldout,
                           int nsplit, int merge, void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);

/* The end of AttentionNCF.forward in one launch (models/attention_ncf.py:208-222): merge of the entry-split attention's partials
 * (ncf_attn_forward_split with merge = 0: dev_part = its workspace, (B, nsplit, UE + 4) floats — [m, l, -, -, O...]) into the user
 * embeddings (+ dev_ubias = UserEmbeddings' bias), cat(candidate_emb, user_emb) (:219), then the MLP of util.py:5-18
 * (EA + UE -> N1 -> N2 -> 1, ReLU between, none after the last).  dev_part == NULL: dev_user holds finished (B, UE) rows.
 * Weights: W1 (N1, EA + UE), W2 (N2, N1), w3 (N2) — weights_packed = 0: W1 / W2 in the reference's own row-major layout;
 * weights_packed = 1: each packed once per weight version by ncf_attn_tail_pack_weight (MFMA operand order: a wave's weight load is
 * one contiguous 1 KB run instead of 16 rows x 64 bytes — 12.8 -> 9.8 us at BASELINE config 3; bit-identical results).  Replaces
 * attn_combine + the fused scoring kernel for evaluation batches (16 pairs per workgroup instead of 32: twice the workgroups).
 * Shapes: ncf_attn_tail_supported (EA = UE in {64, 128}, N1 = 256, N2 = 128); else NCF_EUNSUPPORTED (use ncf_score_fused). */
int ncf_attn_tail_supported(int EA, int UE, int N1, int N2);
int ncf_attn_tail_pack_weight(const float* dev_W, int N, int K, float* dev_packed, ncf_stream_t stream);
int ncf_attn_tail(const float* dev_cand_emb, int64_t ldcand, int EA,
                  const float* dev_part, int nsplit, const float* dev_user, int64_t lduser, int UE, const float* dev_ubias,
                  const float* dev_W1, const float* dev_b1, int N1, const float* dev_W2, const float* dev_b2, int N2,
                  const float* dev_w3, float b3, int weights_packed, float* dev_out, int64_t B, ncf_stream_t stream);

/* Cross-product form of K3 for MANY users against ONE ranked list (full-catalogue top-K and ranks; the reference scores one user
 * per request, webapp/backend.py:78-121, through models/attention_ncf.py:154-216).  The attention logit of a (candidate, rated item)
 * pair never depends on the user, so the logits of a catalogue are one table per weight version:
 *
 * ncf_attn_logits   dev_st[e * ldst + i] = logit of candidate i < I_c against rated item e < I_r (fp32, ldst >= I_c; padding columns
 *     are not written).  Modes and operand conventions exactly as ncf_attn_forward: dev_pc (I_c, A) carries the bias b0, dev_pr
 *     (I_r, A); NCF_ATT_MLP b1 + sum_a w1[a] relu(pc + pr); NCF_ATT_MLP_SCALED the same on the 2^-64 / 2^64 scaled operands with relu
 *     as the [0, 1] clamp; NCF_ATT_COS the dot of the already normalised rows; NCF_ATT_LINEAR (A = 1) pc + pr.  TRANSPOSED on
 *     purpose: for a fixed rated item, 64 consecutive candidates are one 256-byte load.  Every logit is one fmaf chain over
 *     a = 0 .. A-1 in that order (+ b1 last): the table is bitwise independent of the tiling and of I_c / I_r.  No alignment needed.
 *
 * ncf_attn_cross    dev_out[(u * I + j) * ldout + f] = bias[f] + sum_e softmax_e(ST[col_e, cand_j]) val_e feat[col_e, f]
 *     for the listed users u < U and the columns j < I of the ranked list: the user_emb of pair (u, j), the quantity
 *     ncf_attn_forward writes for that pair.  The users' rated sets are a CSR of n_rows rows (dev_rowptr int64, dev_col int32 = rows
 *     of dev_st and of dev_feat, dev_val); dev_user_rows (U,) int64 = the CSR row of each listed user (repeats, any order);
 *     dev_cand_ids (I,) int64 = the columns of dev_st that are ranked, or NULL for 0 .. I-1 (then I <= I_c); dev_feat (I_r, Fdim)
 *     the projected rows rated_items @ Wu^T, dev_out_bias (Fdim) or NULL.  An entry with col outside [0, I_r) is masked; an empty or
 *     fully masked row (and a row whose logits are all -inf: softmax denominator 0) gives exactly the bias bits; a dev_user_rows or
 *     dev_cand_ids value out of range sets *dev_oob_flag (sticky, may be NULL) and that pair's row is written as the bias.
 *     One workgroup per (user, 128 candidates): the exact row maximum first, then exp / sum / aggregation per tile of entries
 *     with the aggregation on v_mfma_f32_32x32x2_f32; no atomics, one fixed summation order: bitwise repeatable.
 *     Shapes: ncf_attn_cross_supported(Fdim) = 1 for Fdim % 32 == 0, 32 <= Fdim <= 256, else NCF_EUNSUPPORTED (as the call then
 *     returns; nothing is launched).  ncf_attn_cross_plan names what a call would launch, host only: *nb = Fdim / 32 (the kernel
 *     instance attn_cross_kernel<nb, entry_tile>), *entry_tile = entries per staged tile (64 for nb <= 4, else 32), *lds_bytes,
 *     *grid_x = U * ceil(I / 128); any output pointer may be NULL; status as ncf_attn_cross's for the shape. */
int ncf_attn_logits(int mode, const float* dev_pc, int64_t ldpc, int64_t I_c, const float* dev_pr, int64_t ldpr, int64_t I_r, int A,
                    const float* dev_w1, float b1, float* dev_st, int64_t ldst, ncf_stream_t stream);
int ncf_attn_cross_supported(int Fdim);
int ncf_attn_cross_plan(int Fdim, int64_t U, int64_t I, int* nb, int* entry_tile, int64_t* lds_bytes, int64_t* grid_x);
int ncf_attn_cross(const float* dev_st, int64_t ldst, int64_t I_r, int64_t I_c,
                   const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t n_rows,
                   const int64_t* dev_user_rows, int64_t U, const int64_t* dev_cand_ids, int64_t I,
                   const float* dev_feat, int64_t ldfeat, int Fdim, const float* dev_out_bias,
                   float* dev_out, int64_t ldout, int32_t* dev_oob_flag, ncf_stream_t stream);

/* Explanations from the logit table (csrc/attn_explain.hip): for U listed users x k winners each, the rated items whose attention
 * weight exceeds the user's threshold — the `because` / `attention` columns of webapp/backend.py:105-121 — without a dense
 * (U * k, I_c) weight matrix.  dev_st / ldst / I_r / I_c and the CSR (dev_rowptr, dev_col, dev_val, n_rows) exactly as
 * ncf_attn_cross reads them; dev_user_rows (U,) int64; dev_items (U, k) int64 columns of dev_st, -1 = an empty slot (what a top-K
 * result holds past its count); dev_thr (U,) fp32, one threshold per LISTED user (the kernel does not own the threshold rule);
 * max_reasons = E, 1 <= E <= ncf_attn_explain_max_reasons() = 64.  Outputs, contiguous: dev_reason_col (U, k, E) int32,
 * dev_reason_w (U, k, E) fp32, dev_reason_val (U, k, E) fp32 (the rating stored for that entry), dev_reason_cnt (U, k) int32.
 * For the pair (u, s) with candidate c = items[u, s]:
 *   - the valid entries of the user's row are those with 0 <= col_e < I_r; their weights are w_e = exp(ST[col_e, c] - m) / l with m
 *     the exact maximum (taken before any exponential) and l the sum in one fixed order; w_e is a function of the entry's logit, m
 *     and l alone, so equal logits give bit-equal weights;
 *   - an entry qualifies when w_e > thr[u], compared in fp32 on the value that is written; a NaN weight never qualifies;
 *   - reason_cnt = the number of qualifying entries, NOT capped at E;
 *   - the first min(cnt, E) slots hold the qualifying entries in descending weight, ties to the entry stored earlier in the row
 *     (for rows with ascending columns: the lower catalogue position); every remaining slot is written as (-1, 0, 0);
 *   - an empty slot (-1), an empty or fully masked row and an all -inf column give cnt = 0; so does a user row or a candidate out
 *     of range (other than -1), which also sets *dev_oob_flag (sticky, may be NULL).
 * One wave per pair, four pairs per workgroup; no atomics, every order fixed: two calls on the same inputs give the same bits.
 * Refusals, before anything is launched (ncf_last_error set): NCF_EUNSUPPORTED for E outside 1 .. 64 (and for more than 2^31 - 1
 * workgroups), NCF_EINVAL for negative sizes, ldst < I_c or a NULL buffer (dev_col / dev_val may be NULL for a CSR without
 * entries, dev_st for a table without cells); U == 0 or k == 0 is an empty call. */
int ncf_attn_explain_max_reasons(void);
int ncf_attn_explain(const float* dev_st, int64_t ldst, int64_t I_r, int64_t I_c,
                     const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t n_rows,
                     const int64_t* dev_user_rows, int64_t U, const int64_t* dev_items, int64_t k, const float* dev_thr,
                     int max_reasons, int32_t* dev_reason_col, float* dev_reason_w, float* dev_reason_val,
                     int32_t* dev_reason_cnt, int32_t* dev_oob_flag, ncf_stream_t stream);

/* Item-item attention statistics of a sample file from the logit table (csrc/attn_stats.hip): the two (n_items, n_items) tables the
 * reference's eval_model accumulates on the host from dense (batch, catalogue) weight matrices (eval.py:101-108, 137-143).
 * dev_st / ldst / I_r / I_c and the CSR (dev_rowptr int64, dev_col int32, n_rows) exactly as ncf_attn_explain reads them (the
 * ratings' values are not needed); S samples (dev_user_rows[s], dev_cands[s]), both int64; dev_order (S,) int64 and dev_cand_rowptr
 * (I_c + 1,) int64 together list the samples of each candidate c, order[cand_rowptr[c] .. cand_rowptr[c + 1]), in ascending sample
 * index (a stable sort of dev_cands and the bucket offsets).  dev_sum (I_c, ldsum) float64 and dev_count (I_c, ldcount) int64 are
 * UPDATED IN PLACE; dev_workspace: ncf_attn_stats_workspace_bytes(S) = 8 * S bytes, 8-byte aligned.
 * For a valid entry e (0 <= col_e < I_r) of sample s's row, with c = cands[s]:
 *     w = exp(ST[col_e, c] - m_s) / l_s      sum[c, col_e] += (double)w      count[c, col_e] += 1
 * m_s the exact maximum over the row's valid entries and l_s the sum in ncf_attn_explain's order (per lane in entry order, then the
 * xor butterfly): the fp32 weight is the one ncf_attn_explain reports.  w = 0 when the row has no finite logit or l_s is 0 or NaN
 * (the reference's NaN -> 0); count is structural: a valid stored entry always counts.  A user row or candidate out of range
 * contributes nothing and sets *dev_oob_flag (sticky, may be NULL).
 * Order contract: no floating-point atomics and no fixed-point substitute — each cell is owned by one wave, which adds the fp32
 * weights as float64 in the order the list gives (ascending sample index), starting from the value already in the table.  So two
 * calls on the same inputs give the same bits, and a file accumulated in two calls (first half, then second half) gives the bits
 * of one call on the whole file.  A sample that dev_order lists under a candidate other than its own is skipped, and nothing
 * outside [0, S) is read whatever the two arrays hold.
 * Precondition: the valid columns within one user row are distinct (provider-built rows are).  A repeated column cannot fault; the
 * value of its cell is unspecified.
 * Two launches: one wave per sample for (m_s, l_s); then one wave per (candidate, slab of 512 rated columns) with the slab's
 * accumulators in LDS.  A candidate's chain of samples is serial: the run time is bounded below by the most sampled candidate.
 * Refusals, before anything is launched (ncf_last_error set): NCF_EINVAL for negative sizes, a NULL buffer (dev_col may be NULL for
 * a CSR without entries; dev_st / dev_sum / dev_count for tables without cells), a pointer not aligned to its element, ldst < I_c,
 * ldsum < I_r or ldcount < I_r; NCF_EUNSUPPORTED for I_r > 2^31 - 1, I_c * ceil(I_r / 512) > 2^31 - 1 or S > 4 * (2^31 - 1);
 * NCF_EWORKSPACE for a short workspace.  S == 0 is an empty call (NCF_OK before any pointer is looked at). */
size_t ncf_attn_stats_workspace_bytes(int64_t S);
int ncf_attn_stats(const float* dev_st, int64_t ldst, int64_t I_r, int64_t I_c,
                   const int64_t* dev_rowptr, const int32_t* dev_col, int64_t n_rows,
                   const int64_t* dev_user_rows, const int64_t* dev_cands, int64_t S,
                   const int64_t* dev_order, const int64_t* dev_cand_rowptr,
                   double* dev_sum, int64_t ldsum, int64_t* dev_count, int64_t ldcount, int32_t* dev_oob_flag,
                   void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);

/* Dense user_matrix -> CSR with shared rows, on the stream (no size is read by the host).  The reference passes AttentionNCF.forward a
 * dense (B, I) user_matrix in which a user's row is repeated for each of their samples (datasets/dynamic_datasets.py:24-40,
 * content_providers/dynamic_profiles_provider.py:55-71; one row for every candidate in webapp/backend.py:78-121) and keeps the
 * entries != 0 (models/attention_ncf.py:158).  Two calls around one cumulative sum the caller runs on the stream:
 *   ncf_dense_csr_rows  -> dev_pair_row[b] = the row pair b uses (the smallest pair index with an IDENTICAL row when share_rows != 0
 *                          — found by a row hash and verified element by element —, b itself otherwise) and dev_rowptr (B + 1) =
 *                          [0, entries row 0 will list, entries row 1 will list, ...] (0 for a row that shares another's)
 *   an inclusive cumulative sum over dev_rowptr, IN PLACE, makes it the CSR's rowptr
 *   ncf_dense_csr_fill  -> the representatives' (col, val) in column order at rowptr[b]; dev_col / dev_val must hold rowptr[B]
 *                          entries (B * I is always enough).
 * -0.0 counts as 0 (unrated); a row containing NaN never shares.  workspace: ncf_dense_csr_workspace_bytes(B), 16-byte aligned.
 * A matrix without columns (I == 0) is never read: dev_user_matrix may then be NULL in both calls; its rows are all equal and empty. */
size_t ncf_dense_csr_workspace_bytes(int64_t B);
int ncf_dense_csr_rows(const float* dev_user_matrix, int64_t ld, int64_t B, int64_t I, int share_rows,
                       int64_t* dev_pair_row, int64_t* dev_rowptr, void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);
int ncf_dense_csr_fill(const float* dev_user_matrix, int64_t ld, int64_t B, int64_t I, const int64_t* dev_rowptr,
                       const int64_t* dev_pair_row, int32_t* dev_col, float* dev_val, ncf_stream_t stream);

/* Shared-row CSR -> per-pair CSR on the stream, with AttentionNCF's train-only target mask (csrc/pair_rows.hip).
 * Replaces: SparseRatings.expanded() (repeat_interleave reads the entry count back to the host) and the mask of
 *           models/attention_ncf.py:195-205 as torch ops (two (nnz, E) gathers for torch.isclose) in a training step.
 * Input: a CSR of R shared rows (dev_rowptr (R + 1, int64), dev_col int32, dev_val fp32) and dev_pair_row (B, int64), the row each
 * pair uses.  Two calls around one cumulative sum the caller runs on the stream, as ncf_dense_csr_rows / ncf_dense_csr_fill:
 *   ncf_pair_rows_count -> dev_out_rowptr[0] = 0 and dev_out_rowptr[b + 1] = the length of shared row pair_row[b]; a row outside
 *                          [0, R) counts 0 and sets *dev_oob_flag (when non-NULL)
 *   an inclusive cumulative sum over dev_out_rowptr (B + 1), IN PLACE, makes it the per-pair CSR's rowptr
 *   ncf_pair_rows_fill  -> one wave per pair: the pair's entries, in the shared row's order, copied to dev_out_col / dev_out_val at
 *                          out_rowptr[b].  Both hold `capacity` entries; an entry at or past capacity is not written and sets
 *                          *dev_flag = 1 (the buffers beyond rowptr[B] are never touched).
 *   With dev_cand != NULL the fill also applies the target mask: an entry whose column c is in [0, I) gets out_col = -1 (a dropped
 *   entry for ncf_attn_forward / ncf_attn_backward) when EVERY element e < E of row dev_cand[b * ldcand + e] is close to
 *   dev_rated[c * ldrated + e]; its value is copied anyway.  A column outside [0, I) is copied unchanged and never compared.
 *   "Close" is torch.isclose(cand, rated, rtol, atol) evaluated in fp32, each operation rounded on its own (the multiply is NOT
 *   contracted into the add), with a = the candidate's element and b = the rated item's:
 *       a == b || (isfinite(a) && isfinite(b) && fabsf(a - b) <= atol + fabsf(rtol * b))
 *   (a NaN is close to nothing; +inf is close to +inf only).  The reference calls isclose(..., atol=1e-5): rtol is torch's 1e-5.
 *   E % 4 == 0, E <= 256, both leading dimensions % 4 == 0 and 16-byte aligned tables take 16-byte loads; any other shape a
 *   generic path with the same results.
 * No atomics: the same inputs give the same bits.  B == 0 launches nothing (dev_out_rowptr[0] is then the caller's to set).
 * NCF_EINVAL for a negative size, E < 1, a leading dimension < E, a negative or NaN tolerance or a NULL pointer; NCF_EUNSUPPORTED
 * from B = 2^31.  Neither call launches anything when it refuses. */
int ncf_pair_rows_count(const int64_t* dev_rowptr, int64_t R, const int64_t* dev_pair_row, int64_t B, int64_t* dev_out_rowptr,
                        int32_t* dev_oob_flag, ncf_stream_t stream);
int ncf_pair_rows_fill(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t R, const int64_t* dev_pair_row,
                       int64_t B, const int64_t* dev_out_rowptr, int32_t* dev_out_col, float* dev_out_val, int64_t capacity,
                       const float* dev_cand, int64_t ldcand, const float* dev_rated, int64_t ldrated, int64_t I, int E, float atol,
                       float rtol, int32_t* dev_flag, ncf_stream_t stream);

/* The candidate side of AttentionNCF.forward in one launch — models/attention_ncf.py:150 (ItemEmbeddings on the candidates) and
 * the candidate half of AttentionNet's first Linear (:176-179 with AttentionNet.0.weight split at the cat boundary):
 *     emb = x . Wi^T + bi   (B, N1);     pc = emb . Wc^T + b0   (B, N2)
 * x (B, K) rows of ldx floats (4-byte aligned rows are fine: K = 2094 in the reference's data), Wi (N1, K) rows of ldw floats,
 * Wc contiguous (N2, N1).  With dev_pair_row != NULL a spare workgroup of the same launch also runs ncf_group_pairs_rows on the
 * batch (B, n_rows <= 32768; same outputs, same workspace size: ncf_attn_candidates_workspace_bytes).
 * Shapes: N1 in {64, 128}, N2 % 16 == 0, N2 <= 256 (ncf_attn_candidates_supported); else NCF_EUNSUPPORTED (use ncf_linear_forward). */
int ncf_attn_candidates_supported(int K, int N1, int N2);
size_t ncf_attn_candidates_workspace_bytes(int64_t n_rows);
int ncf_attn_candidates(const float* dev_x, int64_t B, int64_t ldx, int K,
                        const float* dev_Wi, int64_t ldw, const float* dev_bi, int N1,
                        const float* dev_Wc, const float* dev_b0, int N2,
                        float* dev_emb, int64_t ldemb, float* dev_pc, int64_t ldpc,
                        const int64_t* dev_pair_row, int64_t n_rows, int pairs_per_wg,
                        int64_t* dev_grp_ptr, int64_t* dev_pair_ids, int64_t* dev_wg_ptr, int32_t* dev_wg_row,
                        void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* The same launch with ItemEmbeddings' weight PRE-PACKED in MFMA operand order (once per weight version: ncf_attn_candidates_pack
 * into ncf_attn_candidates_pack_floats(K, N1) floats, 16-byte aligned).  Every weight load is then one contiguous 1 KB run straight
 * into operand registers: the kernel fits two workgroups per CU, so the grouping workgroup runs beside a row tile instead of in front
 * of one.  Same arguments otherwise (no ldw), bit-identical emb / pc — except for batches of at most 128 row tiles (B <= 2048), where a
 * row tile's K range is cut over up to 8 workgroups (every CU ingests a piece of Wi instead of a few ingesting all of it) and a short
 * second launch adds the pieces in order: deterministic, another summation order.  workspace (16-byte aligned):
 * ncf_attn_candidates_packed_workspace_bytes(B, N1, n_rows or -1 without grouping). */
size_t ncf_attn_candidates_pack_floats(int K, int N1);
size_t ncf_attn_candidates_packed_workspace_bytes(int64_t B, int N1, int64_t n_rows);
int ncf_attn_candidates_pack(const float* dev_Wi, int64_t ldw, int K, int N1, float* dev_packed, ncf_stream_t stream);
int ncf_attn_candidates_packed(const float* dev_x, int64_t B, int64_t ldx, int K,
                               const float* dev_Wi_packed, const float* dev_bi, int N1,
                               const float* dev_Wc, const float* dev_b0, int N2,
                               float* dev_emb, int64_t ldemb, float* dev_pc, int64_t ldpc,
                               const int64_t* dev_pair_row, int64_t n_rows, int pairs_per_wg,
                               int64_t* dev_grp_ptr, int64_t* dev_pair_ids, int64_t* dev_wg_ptr, int32_t* dev_wg_row,
                               void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* out[r, :] = x[r, :] / max(||x[r, :]||_2, 1e-12) — torch.nn.functional.normalize(p=2, dim=1) of the cosine
 * variant, models/attention_ncf.py:167-168.  The clamp is torch's clamp_min, not fmaxf: a NaN norm stays NaN, so a row holding a
 * NaN comes out all NaN (and a row holding an infinity as 0 with NaN at the infinity). */
int ncf_l2_normalize_rows(const float* dev_x, int64_t ldx, int64_t R, int E, float* dev_out, int64_t ldout,
                          ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fixed user profiles (csrc/user_profiles.hip) — the users of the content form of BasicNCF (FixedProfilesProvider: item_dim =
 * user_dim = F, an item is its feature row) and of the content-based baseline.
 * Replaces: create_user_embedding of create_dataset.ipynb, a Python loop over the users.
 * The ratings are one CSR with a row per user: dev_rowptr (U + 1, int64), the rated items' positions dev_col (int32; every rating
 * kept, ascending within a row as the reference sorts them) and dev_rating (fp32), nnz entries each; dev_avg (U, float64) is the
 * caller's (mean rating + 2.5) / 2 per user; dev_features (I, F) fp32 rows of ldf floats; dev_out (U, F) fp32 rows of ldout floats.
 * THE CONTRACT, per user u (n_u = rowptr[u + 1] - rowptr[u] entries) and column f:
 *       acc = 0.0 (double)
 *       for e in row u, in order:
 *           acc = acc + ((double)rating[e] - avg[u]) * (double)features[col[e], f]      (product rounded, THEN sum rounded: no FMA)
 *       out[u, f] = (float)(acc / (double)n_u)
 *   — numpy's ((r - avg).reshape(-1, 1) * feat[col]).mean(axis=0) in float64, rounded to fp32, bit for bit.  A row is never split:
 *   no atomics, no reduction across lanes; the same inputs give the same bits.
 * An empty row writes zeros.  A column outside [0, I) sets the sticky *dev_oob_flag (when non-NULL) and that entry adds nothing
 * (n_u still counts it); a row pointer outside [0, nnz] or a decreasing pair sets the flag too and the row is treated as empty.
 * 16-byte accesses when F, ldf and ldout are multiples of 4 and both tables are 16-byte aligned, single floats otherwise (any F >= 1).
 * U == 0 launches nothing.  NCF_EINVAL, before any launch, for a negative U / I / nnz, F <= 0, ldf < F, ldout < F, a NULL
 * rowptr / avg / out with U > 0, a NULL col / rating with nnz > 0 or a NULL feature table with nnz > 0 and I > 0.
 * ------------------------------------------------------------------------------------------------ */
int ncf_user_profiles(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_rating, int64_t nnz, const double* dev_avg,
                      int64_t U, const float* dev_features, int64_t I, int64_t ldf, int F, float* dev_out, int64_t ldout,
                      int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * KernelMF (csrc/kmf.hip) — the collaborative-filtering baseline of the reference's evaluation: biased matrix factorisation
 *       r^ = mu + b_u + b_i + p_u . q_i
 * fitted by per-sample SGD, the linear kernel of the matrix_factorization package (cf_baseline.py).  Replaces: that package's
 * fitting loop (numba on the host), which nothing on the device can run.
 * Tables: dev_PU (U, ldu) and dev_QI (I, ldq) fp32; columns 0 .. F-1 of a row are the factors, column F is the row's bias (b_u in the
 * user's row, b_i in the item's), 1 <= F <= 256, ld >= F + 1.  Columns beyond F are never written.  16-byte accesses when both
 * leading dimensions are multiples of 4 and both tables are 16-byte aligned, single floats otherwise.
 * Stratified SGD (DSGD): users and items are dealt to W blocks each (dev_user_block (U,), dev_item_block (I,), int32); stratum s is
 * the blocks (a, (a + s) mod W), a = 0 .. W-1, which share no user row and no item row.  The samples dev_user / dev_item (int32) and
 * dev_rating (fp32), n of each, are stored stratum-major: block s * W + a holds the samples whose user block is a and whose item
 * block is (a + s) mod W, at dev_block_ptr[s * W + a] .. dev_block_ptr[s * W + a + 1] (int64, W * W + 1 entries).  1 <= W <= 1024.
 * One call enqueues n_epochs * W launches; launch (e, s) is W workgroups of one wave, wave a walks block (s, a) in stored order.  A
 * launch boundary is the only hand-off between strata; within a launch a wave reads and writes the rows of its own block only.
 * THE CONTRACT, per sample (u, i, r) of a block, in stored order, all in fp32 with every product and sum rounded on its own (no FMA):
 *       column c (0 <= c < F) belongs to lane (c / 4) mod 64
 *       part_l = +0.0f;  for the lane's columns in ascending order:  part_l = part_l + p[c] * q[c]
 *       dot    = balanced tree over lanes 0..63 in lane order: adjacent pairs first, then pairs of pairs, ... (6 levels)
 *       pred   = ((mu + bi) + bu) + dot
 *       err    = pred - r
 *       bu'    = bu - lr * (err + reg * bu)
 *       bi'    = bi - lr * (err + reg * bi)
 *       for every c:  p'[c] = p[c] - lr * (err * q[c] + reg * p[c])
 *                     q'[c] = q[c] - lr * (err * p[c] + reg * q[c])      (both from the OLD p[c], q[c])
 *   — the update of the package's linear kernel; the fitting loop does not clip.  The blocks of a stratum touch disjoint rows, so
 *   the result is the one of ANY sequential order of them: the same inputs give the same bits.
 * The kernel checks its own inputs, never dereferences an unchecked id, and a flagged case writes nothing for that sample:
 *       bit 0 of the sticky *dev_flag: an id outside [0, U) / [0, I) — the sample is skipped
 *       bit 1: user_block[u] != a or item_block[i] != (a + s) mod W — the sample is skipped
 *       bit 2: a block_ptr pair that decreases or lies outside [0, n] — the block is treated as empty
 * Loss: wave a keeps sse = sum of (double)err * (double)err over its block, added sequentially from 0.0, and after the block lane 0
 * does dev_sse[e * W + a] = dev_sse[e * W + a] + sse (a plain read-modify-write: launch order makes it the only writer).  dev_sse
 * (n_epochs * W doubles, zeroed by the caller) and dev_flag may be NULL.
 * n == 0 or n_epochs == 0 launches nothing.  NCF_EINVAL, before any launch, for a negative U / I / n / n_epochs, F <= 0,
 * ld < F + 1, W outside 1 .. 1024, a NULL table or plan array, NULL samples with n > 0, a non-finite lr or reg; NCF_EUNSUPPORTED
 * for F > 256.
 * ------------------------------------------------------------------------------------------------ */
#define NCF_KMF_FLAG_ID 1
#define NCF_KMF_FLAG_BLOCK 2
#define NCF_KMF_FLAG_PTR 4
int ncf_kmf_epoch(float* dev_PU, int64_t ldu, int64_t U, float* dev_QI, int64_t ldq, int64_t I, int F,
                  const int32_t* dev_user, const int32_t* dev_item, const float* dev_rating, int64_t n,
                  const int64_t* dev_block_ptr, const int32_t* dev_user_block, const int32_t* dev_item_block, int W,
                  float mu, float lr, float reg, int n_epochs, double* dev_sse, int32_t* dev_flag, ncf_stream_t stream);
/* Fold-in (the package's update_users): fits the rows of dev_PU of the users dev_users[k] (int32, n_users of them, no user twice)
 * against a FIXED dev_QI, n_epochs passes over the user's ratings, which are row k of a CSR: dev_rowptr (n_users + 1, int64),
 * dev_col (item positions, int32) and dev_rating (fp32), nnz entries each.  One wave per user, one launch; per sample THE CONTRACT of
 * ncf_kmf_epoch without the q' and bi' lines.  dev_QI is never written and users not listed keep their rows.  Flags: bit 0 for a user
 * or an item outside its table (the user's whole row, or that sample, is skipped), bit 2 for a row pointer pair that decreases or
 * lies outside [0, nnz] (the row is treated as empty).  dev_sse[e * n_users + k], when non-NULL, is SET to the user's sum of
 * (double)err * (double)err of pass e.  n_users == 0 or n_epochs == 0 launches nothing; the refusals are ncf_kmf_epoch's, with
 * n_users / nnz for n, and NULL pointers refused only where their arrays are non-empty. */
int ncf_kmf_fold_users(float* dev_PU, int64_t ldu, int64_t U, const float* dev_QI, int64_t ldq, int64_t I, int F,
                       const int32_t* dev_users, int64_t n_users, const int64_t* dev_rowptr, const int32_t* dev_col,
                       const float* dev_rating, int64_t nnz, float mu, float lr, float reg, int n_epochs, double* dev_sse,
                       int32_t* dev_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ItemKNN (csrc/knn.hip) — neighbourhood collaborative filtering, the third baseline NCF models are read against (Sarwar et al.
 * 2001; Surprise KNNBasic, LensKit ItemItem): shrunk cosine similarities of the items over the rating matrix, each item's N nearest
 * neighbours, and scores from the neighbours a user rated.  Replaces: nothing in the reference; a torch composition needs the dense
 * (U, I) matrix and its X^T X, whose summation order is not fixed.
 * Ratings: a user CSR dev_rowptr (U + 1, int64), dev_col (int32 item positions, STRICTLY ASCENDING inside a row) and dev_val (fp32,
 * finite, centred however the caller likes), nnz entries each; and its transpose dev_colptr (I + 1, int64), dev_row (int32 user
 * positions, ascending inside a column) and dev_tval (fp32), nnzT entries each, built by a stable sort of the entries on col.
 * THE CONTRACT, all in fp32, every product, sum, quotient and square root rounded on its own (no FMA; division and sqrtf are the
 * correctly rounded IEEE operations, hipcc's default for fp32 — csrc/knn.hip is built without any fast-math flag):
 *   squared norm of item i (ncf_knn_item_sq), over the entries e = 0, 1, ... of column i in stored order:
 *       part_l = +0.0f;  for e = l, l + 64, l + 128, ... in that order:  part_l = part_l + tval[e] * tval[e]
 *       sq[i]  = balanced tree over lanes 0..63 in lane order: adjacent pairs first, then pairs of pairs, ... (6 levels)
 *   Gram row of item i:  dot[j] = +0.0f and co[j] = 0 for every j; then
 *       for the users u of column i in ascending order, for every entry (j, v_uj) of row u:
 *           dot[j] = dot[j] + v_ui * v_uj;   co[j] = co[j] + 1
 *     (a user holds an item at most once, so the order inside a user is immaterial; the order across users is fixed)
 *   similarity:  n = sqrtf(sq[i]) * sqrtf(sq[j])
 *       s_ij = 0.0f  if j == i, or co[j] < min_support, or n == 0
 *       s_ij = (dot[j] / n) * ((float)co[j] / ((float)co[j] + shrink))  otherwise, and 0.0f unless that is > 0
 *   neighbour table: the N largest s_ij > 0 of item i, ties to the lower j (ncf_topk_rows' order): nb_pos (I, N) int32, -1 past the
 *       count; nb_sim (I, N) fp32, 0 past the count; nb_cnt (I,) int32
 *   score of (user row u, item i):  num = den = +0.0f; for t = 0 .. nb_cnt[i] - 1 in slot order, with j = nb_pos[i][t], s = nb_sim[i][t]:
 *           if row u holds j with value v:  num = num + s * v;   den = den + s
 *       weighted_average = 1:  num / den if den > 0, else fill;      weighted_average = 0:  num
 *   No float atomics anywhere and one fixed order of every sum: the same inputs give the same bits.
 * ncf_knn_item_sq: one wave per item.  ncf_knn_sim_rows writes the similarity rows of the items [i0, i1) into dev_out (i1 - i0, I)
 * fp32, rows of ldo floats; ncf_topk_rows over those rows selects the table.  One workgroup of one wave per (item, tile of col_tile
 * columns), the tile's dot / co in LDS, a workgroup barrier between two users of the walk; col_tile = 0 chooses (at most 2048),
 * otherwise a multiple of 64 up to 8192.  Every id is checked before it is dereferenced: a user or an item outside [0, U) / [0, I)
 * or a pointer pair that decreases or leaves its array sets the sticky *dev_oob_flag (when non-NULL) and that entry (row, column) adds
 * nothing; a row of the user CSR whose columns do not strictly ascend sets the sticky *dev_order_flag (when non-NULL; the result of
 * such a row is unspecified, no address leaves the arrays).
 * ncf_knn_scores: the listed rows dev_users (B, int64) of ANY ratings CSR of R rows over the same items (not only the fitted one)
 * against the items [i0, i1), into dev_out (B, i1 - i0) fp32 rows of ldo floats.  One workgroup per (user, 256 items), one lane per
 * item, each neighbour looked up in the user's row by binary search; a row of at most stage_cap entries is staged in LDS first
 * (stage_cap = 0: 2048; at most 8192), a longer one is searched in global memory, with the same bits.  A user row outside [0, R)
 * scores as an empty row and sets *dev_oob_flag, as does a table slot outside [0, I) other than -1 (skipped).
 * ncf_knn_predict: the same device function for n pairs (dev_users[k], dev_items[k]) (int64), one lane per pair, into dev_out (n,):
 * predict(u, i) == scores[u, i] bit for bit.  A pair with a row or an item outside its range scores as an empty row and sets the flag.
 * Refusals, before any launch, with the entry's name in ncf_last_error(): NCF_EINVAL for a negative size, an item range outside
 * [0, I), N outside 1 .. 256, min_support < 1, a shrink or fill that is not finite, shrink < 0, weighted_average not 0 or 1, a
 * col_tile that is not a multiple of 64 (or above 8192), a stage_cap outside 0 .. 8192, ldo below the row's width, and a NULL
 * array that the sizes say is read or written; NCF_EUNSUPPORTED for more than 65535 items (sim_rows) or users (scores) in one call.
 * A call with nothing to do (no item, no user, no pair) returns NCF_OK without a launch.
 * ------------------------------------------------------------------------------------------------ */
int ncf_knn_item_sq(const int64_t* dev_colptr, const float* dev_tval, int64_t nnzT, int64_t I, float* dev_sq, int32_t* dev_oob_flag,
                    ncf_stream_t stream);
int ncf_knn_sim_rows(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t U,
                     const int64_t* dev_colptr, const int32_t* dev_row, const float* dev_tval, int64_t nnzT, int64_t I,
                     const float* dev_sq, int64_t i0, int64_t i1, int min_support, float shrink, int col_tile, float* dev_out,
                     int64_t ldo, int32_t* dev_oob_flag, int32_t* dev_order_flag, ncf_stream_t stream);
int ncf_knn_scores(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t R,
                   const int64_t* dev_users, int64_t B, const int32_t* dev_nb_pos, const float* dev_nb_sim, const int32_t* dev_nb_cnt,
                   int64_t I, int N, int64_t i0, int64_t i1, int weighted_average, float fill, int stage_cap, float* dev_out,
                   int64_t ldo, int32_t* dev_oob_flag, ncf_stream_t stream);
int ncf_knn_predict(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t R,
                    const int64_t* dev_users, const int64_t* dev_items, int64_t n, const int32_t* dev_nb_pos, const float* dev_nb_sim,
                    const int32_t* dev_nb_cnt, int64_t I, int N, int weighted_average, float fill, float* dev_out,
                    int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ImplicitALS (csrc/als.hip) — implicit-feedback alternating least squares, the baseline a full-catalogue top-K number is usually
 * asked to beat (Hu, Koren & Volinsky 2008; implicit's AlternatingLeastSquares; the iALS of Rendle et al. 2021).  Replaces: nothing
 * in the reference; a torch composition builds a dense (rows, F, F) tensor of normal matrices whose summation order is not fixed.
 * Ratings: a CSR dev_rowptr (R + 1, int64), dev_col (int32 positions into the fixed table T, STRICTLY ASCENDING inside a row) and
 * dev_val (fp32, finite and >= 0), nnz entries each.  The confidence of a stored entry is 1 + alpha * val, its preference 1.  T is
 * (n_t, F) fp32 with rows of ldt floats, 1 <= F <= 128 (NCF_ALS_MAX_FACTORS); G is (F, F) fp32, contiguous, only its lower
 * triangle is read.  One half-sweep recomputes a row u as x_u = A_u^-1 b_u with
 *       A_u = G + sum over the row's entries of (alpha * val_e) * t_e t_e^T + reg * I,     b_u = sum of (1 + alpha * val_e) * t_e,
 * t_e being T's row at the entry's column; with G = T^T T that is the exact minimiser of the iALS objective in x_u.
 * THE CONTRACT, all in fp32, every product, sum, difference, quotient and square root rounded on its own (no FMA; division and
 * sqrtf are the correctly rounded IEEE operations, hipcc's default for fp32 — csrc/als.hip is built without any fast-math flag):
 *   Gram (ncf_als_gram): the rows of T are taken in chunks of 256 (NCF_ALS_GRAM_ROWS); chunk c holds rows 256 c .. 256 c + 255.
 *       P_c[a][b] = +0.0f;  for the chunk's rows t in ascending order, for a >= b:  P_c[a][b] = P_c[a][b] + t[a] * t[b]
 *       G[a][b] = +0.0f;  for c = 0, 1, ... in that order:  G[a][b] = G[a][b] + P_c[a][b];      G[b][a] = G[a][b]
 *   Row u (ncf_als_solve_rows), its entries e = 0, 1, ..., n - 1 in stored order, cut into segments of 512 (NCF_ALS_SEG):
 *       w_e = alpha * val_e
 *       S_s[a][b] = +0.0f;  for the entries e of segment s in stored order, for a >= b:  S_s[a][b] = S_s[a][b] + (w_e * t_e[a]) * t_e[b]
 *       A[a][b] = G[a][b];  for s = 0, 1, ... in that order:  A[a][b] = A[a][b] + S_s[a][b];  then  A[a][a] = A[a][a] + reg
 *       b[a] = +0.0f;  for ALL the row's entries e in stored order:  b[a] = b[a] + (1.0f + w_e) * t_e[a]
 *   Cholesky A = L L^T on the lower triangle, for j = 0, 1, ..., F - 1:
 *       s = A[j][j];  for k = 0 .. j - 1 in ascending order:  s = s - L[j][k] * L[j][k];      L[j][j] = sqrtf(s)
 *       for i > j:  v = A[i][j];  for k = 0 .. j - 1 in ascending order:  v = v - L[i][k] * L[j][k];      L[i][j] = v / L[j][j]
 *   forward:   for i = 0 .. F - 1:  v = b[i];  for k = 0 .. i - 1 in ascending order:  v = v - L[i][k] * z[k];      z[i] = v / L[i][i]
 *   backward:  for i = F - 1 .. 0:  v = z[i];  for k = F - 1 .. i + 1 in descending order:  v = v - L[k][i] * x[k];      x[i] = v / L[i][i]
 *   A row without entries is written as zeros, without a solve.  No float atomics anywhere and one fixed order of every sum: the
 *   same inputs give the same bits for any grid, CU count or blocking of the rows.
 * ncf_als_gram: one workgroup per chunk writes P_c into dev_workspace (ncf_als_gram_workspace_bytes(rows, F) bytes: F * F floats
 * per chunk), a second launch adds the chunks in order and mirrors.  rows == 0 gives G = 0.
 * ncf_als_solve_rows: the listed rows dev_rows (B, int64) of ANY such CSR of R rows over T's rows — the ratings by user against the
 * item table, their transpose against the user table, or a foreign CSR against the item table (fold-in of new users).  Row
 * dev_rows[k] is written to row k of dev_out (rows of ldo floats), or to row dev_rows[k] with out_by_row = 1; no other row of dev_out
 * is touched.  One workgroup per listed row: T's rows of 16 entries at a time staged in LDS, the lower triangle of A in registers
 * (tiles of a blocked right-looking elimination, which subtracts the products of every element in exactly the ascending k of the
 * contract), L in an LDS tile of F x F floats, the two substitutions by one wave.  A row of more than one segment does not become a
 * serial chain of its normal matrix: the caller lists its segments, one workgroup per segment writes S_s into dev_scratch, and the
 * row's own workgroup adds them in order — the segment order is the contract, so both forms give the same bits.  The plan:
 * dev_seg_base (B, int64) is the first slot of listed row k in dev_scratch (n_slots slots of F * F floats), -1 for a row of at most
 * one segment; dev_seg_row (n_slots, int64) is the k whose segment a slot holds (slot j holds segment j - dev_seg_base[k]).  Both
 * may be NULL with n_slots == 0, when no listed row is longer than one segment.  The right-hand side b stays one serial sum over
 * the row's entries in the row's own workgroup (64 entries staged at a time where F >= 64: the tile L will take is free until
 * then): that chain is the floor of a half-sweep.
 * The kernels check their own inputs and never dereference an unchecked id; bits of the sticky *dev_flag (when non-NULL):
 *       bit 0: a column outside [0, n_t) — the entry is skipped (it adds nothing to S, A or b)
 *       bit 1: a listed row outside [0, R), a pointer pair that decreases or lies outside [0, nnz], or a plan that does not hold the
 *              row's segments — the row is written as zeros (a listed row outside [0, R) with out_by_row = 1 writes nothing)
 *       bit 2: a row whose columns do not strictly ascend — the row is written as zeros
 *       bit 3: a val that is negative or not finite — the entry is skipped
 *       bit 4: a pivot s that is not > 0 or not finite — the row is written as zeros
 * Refusals, before any launch, with the entry's name in ncf_last_error(): NCF_EINVAL for a negative size, F outside 1 .. 128,
 * ld < F, a reg that is not finite or not > 0, an alpha that is not finite or negative, out_by_row not 0 or 1, a float array that
 * is not 4-byte aligned or an int64 array that is not 8-byte aligned, a workspace that is too small, and a NULL array that the
 * sizes say is read or written.  A call with nothing to do (B == 0) returns NCF_OK without a launch.
 * ------------------------------------------------------------------------------------------------ */
#define NCF_ALS_MAX_FACTORS 128
#define NCF_ALS_GRAM_ROWS 256
#define NCF_ALS_SEG 512
#define NCF_ALS_FLAG_COL 1
#define NCF_ALS_FLAG_PTR 2
#define NCF_ALS_FLAG_ORDER 4
#define NCF_ALS_FLAG_VAL 8
#define NCF_ALS_FLAG_PIVOT 16
size_t ncf_als_gram_workspace_bytes(int64_t rows, int F);
int ncf_als_gram(const float* dev_T, int64_t rows, int64_t ld, int F, float* dev_G, void* dev_workspace, size_t workspace_bytes,
                 ncf_stream_t stream);
int ncf_als_solve_rows(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t R,
                       const int64_t* dev_rows, int64_t B, const float* dev_T, int64_t n_t, int64_t ldt, int F, const float* dev_G,
                       float alpha, float reg, float* dev_out, int64_t ldo, int out_by_row, const int64_t* dev_seg_base,
                       const int64_t* dev_seg_row, int64_t n_slots, float* dev_scratch, int32_t* dev_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * EASE (csrc/ease.hip) — the closed-form item-item baseline (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"):
 *       G = X^T X (I x I, X the U x I rating matrix),   P = (G + lambda 1)^-1,
 *       W[i][j] = -P[i][j] / P[j][j] (i != j),  W[j][j] = 0,       score(u, j) = sum over i of X[u][i] W[i][j].
 * Replaces: nothing in the reference; a torch composition needs the dense (U, I) matrix, X^T X in no fixed order and
 * torch.linalg.inv.  Ratings: ItemKNN's user CSR (columns STRICTLY ASCENDING inside a row) and its transpose, as ncf_knn_sim_rows
 * takes them.  Every dense matrix is fp32 with rows of ld floats, 4-byte aligned, at most 65535 wide.
 * THE CONTRACT (csrc/ease.hip is built with -ffp-contract=off and without any fast-math flag):
 *   Gram (ncf_ease_gram), row i:  G[i][j] = +0.0f for every j; then
 *       for the users u of column i in ascending order, for every entry (j, v_uj) of row u:  G[i][j] = G[i][j] + v_ui * v_uj
 *     each product and each sum rounded on its own; it is ncf_knn_sim_rows' walk (csrc/gram_walk.h).  Two items share their users in
 *     one order, so G == G^T bit for bit.
 *   Inversion (ncf_ease_invert): A[i][i] = A[i][i] + lambda, then A is replaced IN PLACE by its inverse by blocked right-looking
 *     Gauss-Jordan elimination without pivoting, panels K = [k0, k0 + nb) of nb = NCF_EASE_BLOCK in ascending order:
 *       D = A[K][K]^-1 by scalar Gauss-Jordan in fp32 (step k: p = a[k][k]; a[k][j] = a[k][j] / p, a[k][k] = 1 / p;
 *           a[i][k] = -(a[i][k] * (1 / p)); a[i][j] = a[i][j] - a[i][k] * (a[k][j] / p), each operation rounded on its own)
 *       R = D * E (nb x N), E = the rows K of A with the columns K replaced by the identity
 *       A[i][j] = A0[i][j] + sum over k of C[i][k] * R[k][j], A0 = A with the rows K and the columns K zeroed, C = -A[:][K] with the
 *           rows K replaced by the identity — which also leaves R in the rows K, -A[:][K] D in the columns K and D in (K, K)
 *     Every sum over k of R and of the update is ONE chain acc = fmaf(a_k, b_k, acc) in ascending k from the stated start, on
 *     v_mfma_f32_32x32x2_f32: no split-K, no float atomics, so the same input gives the same bits on every run.  The result is NOT
 *     a bit-exact function a host can restate cheaply; tests hold it to the float64 inverse (tests/ease_ref.py).  2 N^3 FLOP.
 *     A pivot p that is not > 0 or not finite sets bit NCF_EASE_FLAG_PIVOT of the sticky *dev_flag (when non-NULL) and the whole
 *     output is written as zeros; the kernels reach their end.
 *   Weights (ncf_ease_weights), IN PLACE:  d[j] = P[j][j] (copied to dev_diag first);  W[i][j] = -(P[i][j] / d[j]) for i != j with
 *     the correctly rounded division, W[j][j] = +0.0f.
 *   Score of (user row u, item j) (ncf_ease_scores, ncf_ease_predict):  s = +0.0f; for the row's entries e in stored order:
 *       s = s + val_e * W[col_e][j],  the product and the sum rounded on their own.
 * ncf_ease_gram writes the rows [i0, i1) of G into dev_G (i1 - i0, I), rows of ldg floats.  A user, an item or a pointer pair
 * outside its array sets the sticky *dev_oob_flag (when non-NULL) and adds nothing; a row of the user CSR whose columns do not
 * strictly ascend sets bit NCF_EASE_FLAG_ORDER of *dev_flag (the result of such a row is unspecified, no address leaves the arrays).
 * ncf_ease_invert: dev_workspace of ncf_ease_invert_workspace_bytes(N) bytes, 256-byte aligned, is scratch (the panel's D, C and R).
 * ncf_ease_scores: the listed rows dev_users (B, int64) of ANY ratings CSR of R rows over the same items against the items [i0, i1),
 * into dev_out (B, i1 - i0) rows of ldo floats.  One workgroup per (user, 1024 columns), lanes own columns; a row of at most
 * stage_cap entries is staged in LDS first (0: 2048; at most 8192), a longer one is read from global memory, with the same bits.  A
 * user row outside [0, R) scores as an empty row and sets *dev_oob_flag; a column id outside [0, I) sets it and adds nothing.
 * ncf_ease_predict: the same device function for n pairs (dev_users[k], dev_items[k]) (int64): predict(u, j) == scores[u, j] bit for
 * bit.  A pair with a row or an item outside its range scores 0 and sets the flag.
 * Refusals, before any launch, with the entry's name in ncf_last_error(): NCF_EINVAL for a negative size, an item range outside
 * [0, I), ld below the width, a lambda that is not finite or not > 0, a stage_cap outside 0 .. 8192, a misaligned array, a NULL array
 * that the sizes say is read or written, and a workspace that is too small; NCF_EUNSUPPORTED for more than 65535 items, or users in
 * one ncf_ease_scores call.  A call with nothing to do returns NCF_OK without a launch.
 * ------------------------------------------------------------------------------------------------ */
#define NCF_EASE_BLOCK 128
#define NCF_EASE_FLAG_ORDER 1
#define NCF_EASE_FLAG_PIVOT 2
int ncf_ease_gram(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t U,
                  const int64_t* dev_colptr, const int32_t* dev_row, const float* dev_tval, int64_t nnzT, int64_t I, int64_t i0,
                  int64_t i1, float* dev_G, int64_t ldg, int32_t* dev_oob_flag, int32_t* dev_flag, ncf_stream_t stream);
size_t ncf_ease_invert_workspace_bytes(int64_t N);
int ncf_ease_invert(float* dev_A, int64_t N, int64_t lda, float lambda, void* dev_workspace, size_t workspace_bytes, int32_t* dev_flag,
                    ncf_stream_t stream);
int ncf_ease_weights(float* dev_P, int64_t N, int64_t ldp, float* dev_diag, ncf_stream_t stream);
int ncf_ease_scores(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t R,
                    const int64_t* dev_users, int64_t B, const float* dev_W, int64_t I, int64_t ldw, int64_t i0, int64_t i1,
                    int stage_cap, float* dev_out, int64_t ldo, int32_t* dev_oob_flag, ncf_stream_t stream);
int ncf_ease_predict(const int64_t* dev_rowptr, const int32_t* dev_col, const float* dev_val, int64_t nnz, int64_t R,
                     const int64_t* dev_users, const int64_t* dev_items, int64_t n, const float* dev_W, int64_t I, int64_t ldw,
                     float* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SLIM (csrc/slim.hip) — the sparse item-item baseline EASE is measured against (Ning & Karypis 2011, "SLIM: Sparse Linear Methods
 * for Top-N Recommender Systems"): the same regression X ~ X W, diag(W) = 0, with an L1 + L2 penalty (and W >= 0) instead of a closed
 * form.  Column j of W minimises
 *       1/2 w^T G w - G[j]^T w + 1/2 l2 |w|^2 + l1 |w|_1,   w[j] = 0   (and w >= 0 when `positive`),     G = X^T X
 * by cyclic coordinate descent on the Gram matrix of ncf_ease_gram; W is scored by ncf_ease_scores / ncf_ease_predict.
 * Replaces: nothing in the reference; on a host it is scikit-learn's ElasticNet once per item, and the torch composition updates
 * all columns at once with one dense rank-1 update of an I x I matrix per coordinate.
 * THE CONTRACT (csrc/slim.hip is built with -ffp-contract=off and without any fast-math flag; the division is the correctly rounded
 * one).  State of a column: w (I) and q = G w (I), both +0.0f at a cold start, and d[k] = G[k][k].  One sweep visits k = 0 .. I - 1
 * in ascending order and skips k == j:
 *       t = d[k] * w[k];  r = q[k] - t;  rho = G[j][k] - r;  den = d[k] + l2
 *       positive:  a = rho - l1;  wn = (a > 0 && den > 0) ? a / den : +0.0f
 *       signed:    rho >  l1 && den > 0 -> (rho - l1) / den
 *                  rho < -l1 && den > 0 -> (rho + l1) / den
 *                  else +0.0f
 *       delta = wn - w[k]
 *       if delta != 0:  for every i: q[i] = q[i] + delta * G[k][i];  w[k] = wn;  steps += 1
 *   every product, sum and quotient rounded on its own.
 *   Stopping: a column stops after the first sweep whose largest |delta| is <= tol, or after max_sweeps.
 *   Warm start (warm != 0): w is taken from the output row, with w[j] = +0.0f, and q is rebuilt as
 *       q = +0;  for k ascending with w[k] != 0:  q = q + w[k] * G[k]
 *     before the first sweep.
 *   Per-column outputs: the row of w, sweeps (int32), steps (int32, the updates with delta != 0) and last (fp32, the largest |delta|
 *     of the last sweep; last > tol says the column met max_sweeps first — there is no error bit for that).
 *   No reduction over floats occurs anywhere in this, so the result is ONE function of the inputs that a host restates bit for bit
 *   (tests/slim_ref.py), sweeps and steps included, whatever the workgroup size.  The kernel screens a block of coordinates side by
 *   side against an unchanged q and applies the first one with delta != 0, which is the one the serial loop would have applied.
 * dev_G: (I, I) fp32, rows of ldg floats.  dev_cols: (n,) int32, the columns to solve, in the order their workgroups start (the host
 * lists the heaviest, by d[j], first).  dev_Wt: (I, ldw) fp32 — row dev_cols[c] receives COLUMN dev_cols[c] of W; rows that are not
 * listed and the floats of a row past I are not touched.  dev_sweeps / dev_steps / dev_last: (n,), indexed by c.  A column outside
 * [0, I) sets the sticky *dev_oob_flag (when non-NULL), touches no row and reports 0 / 0 / +0.0f.  A column listed again is solved
 * once: every listing reports the first listing's three outputs.  q lives in LDS, 4 I bytes of it (above 64 KiB the dynamic-LDS
 * limit is raised): NCF_SLIM_MAX_ITEMS is what fits beside the ballot slots.
 * Refusals, before any launch, with the entry's name in ncf_last_error(): NCF_EINVAL for a negative size, ld below the width, l1 or
 * l2 negative or not finite, tol negative or not finite, max_sweeps < 1, a misaligned array, or a NULL array that the sizes say is
 * read or written; NCF_EUNSUPPORTED for I > NCF_SLIM_MAX_ITEMS.  n == 0 returns NCF_OK without a launch.
 * ------------------------------------------------------------------------------------------------ */
#define NCF_SLIM_MAX_ITEMS 32768
int ncf_slim_solve(const float* dev_G, int64_t I, int64_t ldg, const int32_t* dev_cols, int64_t n, float l1, float l2, int positive,
                   int warm, int max_sweeps, float tol, float* dev_Wt, int64_t ldw, int32_t* dev_sweeps, int32_t* dev_steps,
                   float* dev_last, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Diversified top-K (csrc/mmr.hip) — greedy Maximal Marginal Relevance (MMR) re-ranking of one candidate pool per user, the pools
 * being what ncf_topk_rows / ncf_dot_topk / ncf_mlp_topk return.  Replaces: nothing in the reference, which stops at the relevance
 * list; a torch composition needs a (B, N, N) Gram tensor and K rounds of masked arg-max launches.
 * dev_vec: item vectors (n_items, D) fp32, rows of ldv floats (the similarity is their plain dot product: pass L2-normalised rows
 * for cosines).  dev_score (B, N) fp32 and dev_pos (B, N) int64, contiguous: the pools, slot j of user b at b * N + j; dev_count
 * (B,) int32 slots in use per pool, NULL = N.  Outputs, contiguous: dev_out_slot (B, K) int32, dev_out_value (B, K) fp32,
 * dev_out_count (B,) int32.
 * THE CONTRACT, per user b, independent of every other user:
 *       n = min(count[b], N), N when dev_count is NULL; a negative count is 0
 *       slot j < n is LIVE iff 0 <= pos[j] < n_items and score[j] is finite.  The pool is NOT assumed sorted.
 *       a position >= n_items or < -1 in a slot j < n also sets the sticky *dev_oob_flag (when non-NULL); -1, the padding of the
 *       top-K kernels, sets nothing.  Every position is checked before it is used as an address; a dead slot's row is never read.
 *   relevance:   normalize = 0:  rel_j = score_j
 *                normalize = 1:  rel_j = (score_j - lo) / (hi - lo), lo / hi = the minimum / maximum score over the live slots; two
 *                                subtractions and one division, each one IEEE fp32 operation; rel_j = 0 for all j when hi == lo
 *   similarity:  sim(j, p) = sum over d of vec[pos_j, d] * vec[pos_p, d] in fp32, every product and every sum rounded on its own
 *                (no FMA), summed SEQUENTIALLY in ascending d:
 *       acc = +0.0f;  for d = 0 .. D-1:  acc = acc + vec[pos_j, d] * vec[pos_p, d]
 *   step 0 picks the live slot with the largest rel_j; its value is rel_j.
 *   step t >= 1 picks, among the live slots not picked yet, the largest value
 *       v_j = (lambda * rel_j) - ((1 - lambda) * m_j)           (three operations, each rounded; 1 - lambda once, in fp32)
 *       m_j = the largest sim(j, p) over the slots p picked so far:  m_j starts at -inf, and after each pick  if sim > m_j: m_j = sim
 *   comparator:  a beats b iff  a > b,  or a == b and a's slot is lower,  or b is NaN and a is not,  or both are NaN and a's slot is
 *                lower — ncf_topk_rows' order: ties to the lower column, NaN last.
 *   outputs:     out_count[b] = min(K, number of live slots); for t < out_count[b]: out_slot[b, t] = the slot picked at step t and
 *                out_value[b, t] = its value when picked; past that slot -1 and value -inf.
 *   No atomics, one thread per slot: the same inputs give the same bits.
 * ncf_mmr_supported (host only) answers 1 for 1 <= N <= 256, 4 <= D <= 256 with D % 4 == 0, 1 <= K <= min(N, 128), else 0; outside
 * that envelope ncf_mmr_rerank returns NCF_EUNSUPPORTED.  NCF_EINVAL, before any launch, for a negative B / n_items / N / D / K, a
 * lambda outside [0, 1] or NaN, normalize not 0 or 1, ldv < D, and (with B > 0) a NULL dev_score / dev_pos / output, or a NULL
 * dev_vec with n_items > 0.  B == 0 launches nothing and looks at no pointer.
 * The pool's rows are gathered once into LDS (stride D + 1 words) as far as 160 KiB hold them beside the per-slot state; slots past
 * that (N = 256 with D > 156 only) read their rows from global memory at every step, in the same summation order.  16-byte global
 * reads when ldv is a multiple of 4 and dev_vec is 16-byte aligned, single floats otherwise.
 * ------------------------------------------------------------------------------------------------ */
int ncf_mmr_supported(int N, int D, int K);
int ncf_mmr_rerank(const float* dev_vec, int64_t n_items, int D, int64_t ldv, const float* dev_score, const int64_t* dev_pos,
                   const int32_t* dev_count, int64_t B, int N, int K, float lambda, int normalize, int32_t* dev_out_slot,
                   float* dev_out_value, int32_t* dev_out_count, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Backward (training step).  The reference trains through torch autograd (train.py:95-110); these
 * are the gradient kernels of K1 / K2.  fp32.
 *   dX = dY . W            : ncf_mlp_forward(n_layers = 1) with the transposed weight (no dedicated entry)
 *   dW = dY^T . X          : ncf_gemm_tn(A = dY (M, N1), B = X (M, N2)) -> (N1, N2); ordered split over M, deterministic
 *   db = column sums of dY : ncf_colsum
 *   ReLU                   : ncf_relu_backward zeroes dY where the forward output was <= 0 (ncf_relu_backward_out: into a new buffer)
 *   embedding rows         : ncf_scatter_add_rows  dst[idx[p], :] += src[p, :]  (float atomics: order-dependent last bits)
 * ------------------------------------------------------------------------------------------------ */
/* out = act(x . W^T + b) for ONE layer with the activation selectable (relu != 0 -> ReLU): the single-layer form of
 * ncf_mlp_forward used by the autograd wrappers, which need every layer's output (util.py:12-17 one Linear at a time). */
int ncf_linear_forward(int dtype, const void* dev_x, int64_t M, int64_t ldx, const void* dev_W, const void* dev_b, int K, int N,
                       int relu, void* dev_out, int64_t ldo, ncf_stream_t stream);
/* Which kernel ncf_linear_forward / a layer of ncf_mlp_forward runs for M rows, N outputs and K inputs under the current
 * "linear_kernel" / "linear_kslices" options: the launch rule itself, answered without launching and without touching the
 * device (like ncf_score_fused_partial_in_lds).  Any output pointer may be NULL.
 *   *form        0 nothing (M = 0), 1 LDS-tiled kernel, 2 row-dot kernel (N <= 8), 3 row-streaming kernel, one row tile per
 *                wave ("rs"), 4 persistent row-streaming kernel ("rsp")
 *   *nt          forms 3 / 4: 32-column tiles per wave of the kernel launched (N / 32, or 1 with column blocks); else 0
 *   *kslices     form 3: waves that split K of one row tile (1, 2, 4 or 8); else 1
 *   *col_blocks  gridDim.y: form 3 column blocks of 32 * nt outputs, form 1 blocks of 64 outputs; else 1
 *   *grid_x      gridDim.x
 * NCF_EINVAL for M < 0, N <= 0 or K <= 0. */
int ncf_linear_plan(int64_t M, int N, int K, int* form, int* nt, int* kslices, int* col_blocks, int64_t* grid_x);
size_t ncf_gemm_tn_workspace_bytes(int64_t M, int N1, int N2);
int ncf_gemm_tn(const float* dev_A, int64_t lda, const float* dev_B, int64_t ldb, int64_t M, int N1, int N2,
                float* dev_out, int64_t ldo, void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);
size_t ncf_colsum_workspace_bytes(int64_t M, int N);
int ncf_colsum(const float* dev_X, int64_t ldx, int64_t M, int N, float* dev_out, void* dev_workspace, size_t workspace_bytes,
               ncf_stream_t stream);
int ncf_relu_backward(float* dev_dY, int64_t ld_dY, const float* dev_Y, int64_t ld_Y, int64_t M, int N, ncf_stream_t stream);
/* out = scale * dY where Y > 0, else 0; dY is not written (the gradient autograd hands over may be shared).  scale = 1 is the
 * ReLU backward; with Y = dropout(relu(.)) and scale = 1 / (1 - p) it is the backward of the ReLU and the dropout together. */
int ncf_relu_backward_out(const float* dev_dY, int64_t ld_dY, const float* dev_Y, int64_t ld_Y, float* dev_out, int64_t ld_out, int64_t M,
                          int N, float scale, ncf_stream_t stream);
int ncf_scatter_add_rows(const float* dev_src, int64_t ld_src, const int64_t* dev_idx, int64_t B, int E,
                         float* dev_dst, int64_t ld_dst, int64_t rows, int32_t* dev_oob_flag, ncf_stream_t stream);

/* nn.Linear-layout embeddings (models/basic_ncf.py:25-33: the parameter is W [E, U], Linear(onehot(i)) = W[:, i] + b):
 *   ncf_gather_cols       out[p, e]      = W[e, idx[p]] + b[e]          (forward of a training step: no W^T + b table)
 *   ncf_scatter_add_cols  dW[e, idx[p]] += src[p, e]                    (its gradient, straight into the [E, U] layout)
 * An out-of-range idx reads zeros / is dropped and sets the sticky flag. */
int ncf_gather_cols(const float* dev_W, int64_t ldw, const float* dev_bias, const int64_t* dev_idx, int64_t B, int E,
                    int64_t n_cols, float* dev_out, int64_t ldo, int32_t* dev_oob_flag, ncf_stream_t stream);
int ncf_scatter_add_cols(const float* dev_src, int64_t ld_src, const int64_t* dev_idx, int64_t B, int E,
                         float* dev_dst, int64_t ld_dst, int64_t n_cols, int32_t* dev_oob_flag, ncf_stream_t stream);

/* One torch.optim.Adam update (train.py:55; amsgrad and maximize off) of ONE tensor in a single pass:
 *   g' = g + weight_decay * p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)          (step counts from 1) */
int ncf_adam_step(float* dev_p, const float* dev_g, float* dev_m, float* dev_v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, ncf_stream_t stream);

/* Row-sparse Adam (csrc/adam_rows.hip): the update of ncf_adam_step applied ONLY to the rows a batch touched, from the batch's
 * per-occurrence gradient rows — no table-sized gradient, no float atomics.
 *   dev_p, dev_m, dev_v  id-major [rows, E] buffers with one row stride ld (the buffers behind an id-major embedding weight and
 *                        its two moments)
 *   dev_g                [n, E] gradient rows with stride ld_g: row o is the gradient of occurrence o of the batch (a column
 *                        half of a wider matrix is passed as it is)
 *   dev_sorted_ids       the batch's n ids in ascending order; dev_perm[j] = the occurrence (row of dev_g, in [0, n)) that
 *                        sorted position j came from, NULL = identity
 * Every run of equal ids has one owner, which adds the run's gradient rows and applies one update to row id of p, m, v with
 * the bias corrections of the tensor-wide `step` (host double arithmetic, as ncf_adam_step).  Weight decay therefore reaches
 * touched rows only, and the moments of an untouched row do not decay.  The sum of a run is a fixed function of the sorted
 * input (runs of up to 64 rows: left to right; longer: 64 interleaved shares, then the shares in order — see the file), so
 * two calls on equal inputs give equal bits, and a row touched once gets the bits of ncf_adam_step on that gradient row.
 * 16-byte accesses when E, ld, ld_g are multiples of 4 and every base is 16-byte aligned, single floats otherwise (any
 * E >= 1).  An id outside [0, rows) is skipped and sets the sticky flag (when non-NULL).  n == 0 launches nothing;
 * NCF_EINVAL for step < 1, E <= 0, ld < E, ld_g < E, negative sizes or a NULL p / m / v / ids / g with n > 0. */
int ncf_adam_rows(float* dev_p, float* dev_m, float* dev_v, int64_t ld, int64_t rows, int E, const int64_t* dev_sorted_ids,
                  const int64_t* dev_perm, int64_t n, const float* dev_g, int64_t ld_g, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Negative sampling for pair-wise (BPR) training (csrc/negsample.hip).
 * Replaces: RankingDataset.__getitem__'s per-sample draw — DataFrame.iloc, probs = r ** w / sum(r ** w) over the row's
 *           negatives (_negative_sampling_probs, type 'sum_dynamic'), np.random.choice(negative_movieIds, p=probs) —
 *           datasets/base.py:57-78.
 * The negatives are one CSR with a row per training sample: dev_rowptr (rows + 1, int64), the negatives' item positions
 * dev_neg (int32) and their ratings dev_rating (fp32), nnz = rowptr[rows] entries each.
 *
 * ncf_negative_cdf: dev_cdf (nnz fp32) = each row's normalised inclusive prefix of its weights, np.random.choice's
 *   cdf = cumsum(p); cdf /= cdf[-1].  The weight of an entry is 1 when w == 0 (numpy's 0 ** 0 == 1), powf(r, w) otherwise.
 *   Prefixes are exact integer sums of the weights in 64-bit fixed point against the row's largest weight (2^-S of it, S =
 *   62 - bit length of the row's length: S >= 46 up to 2^16 entries; a positive weight never quantises below one unit), each
 *   divided by the row's total in double and rounded to fp32: every row is non-decreasing, ends in exactly 1.0f, and an entry
 *   of weight 0 repeats its predecessor's value (a leading one is 0.0f).  A row whose fp32 sum of weights is not finite and
 *   positive (an empty row, all weights 0, a NaN or an overflow) sets *dev_flag = 1 and gets the uniform prefix (k + 1) / n.
 *   Rows of any length; one wave per row.  NCF_EINVAL for w < 0 or NaN, rows < 0 or a NULL pointer.
 * ncf_sample_negatives: one draw per listed sample.  Sample b < n uses row r = dev_pick[b] and slot s = slot0 + b:
 *       x = lowbias32((uint32)s * 0x9E3779B1 ^ seed)
 *       x = lowbias32(x ^ (uint32)(s >> 32) * 0x85EBCA77 ^ 0x68E31DA4)
 *       u = (x >> 8) * 2^-24                                  (exact in fp32, in [0, 1))
 *   with lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32 arithmetic; the mix of
 *   the dropout masks of ncf_spmm_csr_dropout / ncf_attn_forward_dropout).  j = the number of entries of row r's CDF that are
 *   <= u (searchsorted(cdf_row, u, side='right'), at most the row's length - 1), and dev_out[b] = dev_neg[rowptr[r] + j] (int64).
 *   A pick outside [0, rows) or an empty row writes -1 and sets *dev_oob_flag (when non-NULL).  No atomics: the same inputs
 *   give the same bits.  n == 0 launches nothing; NCF_EINVAL for negative sizes, slot0 < 0 or a NULL pointer.
 * Neither call launches anything when it refuses.
 * ------------------------------------------------------------------------------------------------ */
int ncf_negative_cdf(const int64_t* dev_rowptr, int64_t rows, const float* dev_rating, float w, float* dev_cdf, int32_t* dev_flag,
                     ncf_stream_t stream);
int ncf_sample_negatives(const int64_t* dev_rowptr, const float* dev_cdf, const int32_t* dev_neg, int64_t rows, const int64_t* dev_pick,
                         int64_t n, uint32_t seed, int64_t slot0, int64_t* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Unseen negatives for implicit-feedback training and sampled evaluation (csrc/unseen.hip).
 * Provides: the sampling of He et al. 2017 (Neural Collaborative Filtering, sections 3.1 and 4.1) — K items a user has not
 *           interacted with per positive, redrawn every epoch; 99 such items per user as the candidates of leave-one-out
 *           evaluation.  The reference has neither.
 * The seen items are one CSR over users: dev_seen_rowptr (users + 1, int64, a valid CSR over dev_seen_col) and the item positions
 * dev_seen_col (int32), strictly ascending inside a row.
 *
 * THE CONTRACT (tests/unseen_ref.py restates it in numpy).  Row b < n of dev_out (n x K, int64, row-major) belongs to user
 * u = dev_pick[b] and slot s = slot0 + b.  With A the user's seen row, a its length and M = n_items - a, in uint32 arithmetic
 * unless said otherwise:
 *       x   = lowbias32((uint32)s * 0x9E3779B1 ^ seed)
 *       x   = lowbias32(x ^ (uint32)(s >> 32) * 0x85EBCA77 ^ 0x68E31DA4)          (the two rounds of ncf_sample_negatives above)
 *       h_j = lowbias32(x ^ (uint32)(j + 1) * 0xC2B2AE35)                          j = 0 .. K - 1
 *       r_j = ((uint64)h_j * (uint64)(M - j)) >> 32                                in [0, M - j)
 *       dev_out[b, j] = the r_j-th smallest (0-based) element of [0, n_items) \ (A u {dev_out[b, 0 .. j - 1]})
 *   The draws of a row are distinct and never seen.  Draw j is uniform over the M - j items that are left up to the bias of the
 *   multiply-shift: the probabilities of two of them differ by at most 2^-32, so each is within a relative (M - j) / 2^32 of
 *   1 / (M - j) (2^-20 at 4096 items left; at most 1/2).  No rejection and no data-dependent retry: every loop
 *   has a bound known before it starts (j <= K, binary or 64-way searches over a), so no input can make a wave spin.  No float
 *   arithmetic and no atomics.  The result depends only on (seed, s, j, A, n_items): a batch drawn in pieces with advancing slot0
 *   gives the bits of one call, and every launch form gives the same bits.
 * Launch forms: K <= NCF_UNSEEN_LANE_K one lane per row with the row's draws in registers; above, one wave per row with them in
 *   LDS (8 K bytes per wave).
 * Device-side refusals write -1 across the row's K outputs and set the sticky *dev_flag (each condition owns one byte of the
 * word, which a plain byte store sets):
 *       NCF_UNSEEN_FLAG_PICK   a pick outside [0, users)
 *       NCF_UNSEEN_FLAG_FEW    K > M: the user has fewer unseen items than the draws asked for (or a pointer pair that decreases)
 *   On a seen row that does not ascend strictly the output is unspecified but stays in [0, n_items), and the loops still end.
 * n == 0 returns NCF_OK without a launch.  NCF_EINVAL, with ncf_last_error() set and nothing launched: K outside 1 ..
 * NCF_UNSEEN_MAX_K, n_items outside 1 .. 2^31 - 1, a negative users, n or slot0, a NULL dev_seen_rowptr or dev_flag, a NULL
 * dev_pick or dev_out with n > 0 (dev_seen_col may be NULL when no user has seen anything).
 * ------------------------------------------------------------------------------------------------ */
#define NCF_UNSEEN_MAX_K 1024
#define NCF_UNSEEN_LANE_K 8
#define NCF_UNSEEN_FLAG_PICK 1
#define NCF_UNSEEN_FLAG_FEW 256
int ncf_sample_unseen(const int64_t* dev_seen_rowptr, const int32_t* dev_seen_col, int64_t users, int64_t n_items,
                      const int64_t* dev_pick, int64_t n, int K, uint32_t seed, int64_t slot0, int64_t* dev_out /* n x K */,
                      int32_t* dev_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-row top-K with exclusion — the ranking step of a recommendation request.
 * Replaces: DataFrame.sort_values(by='score', ascending=False).iloc[:k] over the whole score vector after
 *           item_features.drop(user_ratings.index) — webapp/backend.py:84, 113-118.
 * dev_scores: (rows, cols) fp32, row-major, leading dimension ld >= cols; never written.
 * dev_seen_rowptr (rows + 1, int64) / dev_seen_col (int32): optional CSR of the columns each row must skip (both NULL = none);
 *   ids need not be sorted, duplicates and ids outside [0, cols) are ignored.
 * Per row: dev_out_score / dev_out_idx (rows, k) — the first out_count[row] = min(k, cols - excluded) entries are the row's best
 *   columns in the order of torch.sort(descending=True, stable=True) over the remaining columns (equal scores: lower column
 *   first; -0.0 == +0.0; NaN below every number including -inf, NaNs by column); the remaining slots hold idx -1, score -inf.
 *   Scores are the input's bits.  Deterministic: no atomics decide an order.
 * Supported: 1 <= k <= 1024 (NCF_EINVAL otherwise), 1 <= cols <= 2^24 and rows <= 65536 (NCF_EUNSUPPORTED otherwise); nothing is
 *   launched on a refusal.  Rows longer than 8192 columns are split over workgroups (per-tile candidates in the workspace, then a
 *   merge launch); the workspace (ncf_topk_workspace_bytes; 16-byte aligned; 0 bytes for cols <= 8192) is bounded by processing
 *   the rows in chunks.
 * ------------------------------------------------------------------------------------------------ */
size_t ncf_topk_workspace_bytes(int64_t rows, int64_t cols, int k);
int ncf_topk_rows(const float* dev_scores, int64_t rows, int64_t cols, int64_t ld, const int64_t* dev_seen_rowptr,
                  const int32_t* dev_seen_col, int k, float* dev_out_score, int32_t* dev_out_idx, int32_t* dev_out_count,
                  void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused dot-product top-K (csrc/dot_topk.hip) — "rank every item for these users" for a dot-product readout (MF, GraphNCF with
 * use_dot_product=True): ncf_gather_dot over every (user, item) pair followed by ncf_topk_rows, without the B x I score matrix.
 * For each row r < rows (user row a = tabA[idxA[r]], or tabA[r] with idxA NULL) and each column c < cols of the ranked list (item
 * row tabB[idxB[c]], or tabB[c] with idxB NULL), score(r, c) = <a, tabB[..]> over D fp32 elements, BIT-IDENTICAL to what
 * ncf_gather_dot (NCF_F32) returns for that pair: 16 fmaf chains (chain s over e = s, s+16, ... in increasing e, from +0.f), then
 * q_l = p_l + p_{l+8}, r_l = q_l + q_{l+4}, t_l = r_l + r_{l+2}, score = t_0 + t_1.  The output is ncf_topk_rows' over that
 * score matrix: per row the k best columns by the 64-bit key (map(score) << 32 | ~c) — descending score, ties to the lower
 * column, NaN last — skipping the columns listed for the row in the optional CSR (dev_seen_rowptr (rows + 1) int64,
 * dev_seen_col int32; unsorted, duplicates and ids outside [0, cols) ignored).  dev_out_score / dev_out_idx: rows x k,
 * dev_out_count: rows; slots past the count hold idx -1 and score -inf.  An output score is recovered from its key: the caller's
 * bits for every non-NaN score; a NaN score ranks last but its payload is not kept.
 * Out-of-range ids in idxA / idxB read as zero rows and set *dev_oob_flag (when non-NULL), as in ncf_gather_dot.
 * Supported: 1 <= k <= 128 and 1 <= D <= 256 (the fused kernel's limits; NCF_EUNSUPPORTED otherwise, and for k outside the ABI
 *   range 1 .. 1024 NCF_EINVAL: take ncf_gather_dot + ncf_topk_rows, which give the same answer), 1 <= cols <= 2^24, rows <= 65536;
 *   ldA, ldB >= D.  Nothing is launched on a refusal.  The workspace (ncf_dot_topk_workspace_bytes, 16-byte aligned, never 0 for
 *   rows > 0) holds k keys per row and column tile; rows are processed in chunks that keep it near 256 MB.  No host
 *   synchronisation: the call captures into a HIP graph.
 * ------------------------------------------------------------------------------------------------ */
size_t ncf_dot_topk_workspace_bytes(int64_t rows, int64_t cols, int D, int k);
int ncf_dot_topk(const float* dev_tabA, int64_t rowsA, int64_t ldA, const float* dev_tabB, int64_t rowsB, int64_t ldB,
                 const int64_t* dev_idxA, const int64_t* dev_idxB, int64_t rows, int64_t cols, int D, const int64_t* dev_seen_rowptr,
                 const int32_t* dev_seen_col, int k, float* dev_out_score, int32_t* dev_out_idx, int32_t* dev_out_count,
                 void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused MLP top-K (csrc/mlp_topk.hip) — "rank every item for these users" for an MLP readout (BasicNCF: cat(user, item);
 * GraphNCF with use_dot_product=False: cat(item, user)): ncf_score_fused over every (user, item) pair followed by ncf_topk_rows,
 * without the pair id columns or the B x I score matrix.  The concat's first part (EA wide) comes from dev_tabA, the second (EB
 * wide) from dev_tabB; user_first != 0 says the user is the first part (rows of tabA, items rows of tabB), 0 that the item is
 * (items rows of tabA, users rows of tabB).  Row r < rows is user dev_user_ids[r] (r with NULL), column c < cols of the ranked
 * list is item dev_item_ids[c] (c with NULL).  score(r, c) is BIT-IDENTICAL to what ncf_score_fused (NCF_F32) returns for that
 * pair with the same packed blob (ncf_mlp_pack; n_layers, dims as there): the first part's share of layer 1 runs once per row
 * of the first part (in the fused scorer's operation order) instead of once per pair.  The output is ncf_topk_rows' over that
 * score matrix, as in ncf_dot_topk: keys (map(score) << 32 | ~c), ties to the lower column, NaN last, the columns listed for the
 * row in the optional CSR (dev_seen_rowptr (rows + 1) int64, dev_seen_col int32; duplicates and ids outside [0, cols) ignored)
 * skipped; out_score / out_idx rows x k, out_count rows, slots past the count idx -1 / score -inf.  Scores are recovered from
 * keys: the caller's bits for every non-NaN score (a fused-MLP score is never -0.0); a NaN ranks last, its payload not kept.
 * Out-of-range user or item ids read as zero rows and set *dev_oob_flag (when non-NULL), as in ncf_score_fused.
 * Supported (ncf_mlp_topk_supported): dtype NCF_F32, a (K0 = EA + EB, dims) shape with an ncf_score_fused instance, EA and EB
 *   both >= 8 and multiples of 8, 1 <= k <= 128; NCF_EUNSUPPORTED otherwise (k outside the ABI range 1 .. 1024: NCF_EINVAL) —
 *   take ncf_score_fused + ncf_topk_rows, which give the same answer.  1 <= cols <= 2^24, rows <= 65536; tables 16-byte aligned
 *   with ld % 4 == 0.  Nothing is launched on a refusal.  The workspace (ncf_mlp_topk_workspace_bytes, 16-byte aligned, never 0
 *   for rows > 0) holds the first part's layer-1 state (dims[1] floats per user, or per column when user_first == 0) and k keys
 *   per row and column range; rows are processed in chunks that keep the key part near 256 MB.  No host synchronisation: the
 *   call captures into a HIP graph.
 * ------------------------------------------------------------------------------------------------ */
int ncf_mlp_topk_supported(int dtype, int EA, int EB, int n_layers, const int* dims, int k);
size_t ncf_mlp_topk_workspace_bytes(int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims, int k);
int ncf_mlp_topk(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, const void* dev_tabB, int64_t rowsB, int64_t ldB,
                 int EA, int EB, int user_first, const int64_t* dev_user_ids, const int64_t* dev_item_ids, int64_t rows,
                 int64_t cols, int n_layers, const int* dims, const void* dev_packed, const int64_t* dev_seen_rowptr,
                 const int32_t* dev_seen_col, int k, float* dev_out_score, int32_t* dev_out_idx, int32_t* dev_out_count,
                 void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exact full-catalogue ranks (csrc/rank.hip, csrc/mlp_topk.hip) — where each held-out column of a row stands among ALL of the row's
 * non-excluded columns: the quantity behind HR@K / Recall@K / NDCG@K / MRR / AUC.  Siblings of the three top-K entry points, with
 * the same tables, ids, exclusion CSR, key order and bit-identity of the scores; no candidate buffer, merge level or sort.
 * Targets: a CSR (dev_tgt_rowptr (rows + 1) int64, dev_tgt_col int32 of n_targets entries in all) of columns of the ranked list.
 *   The kernels address entry e = rowptr[r] + i of row r in dev_tgt_col and dev_rank, so a slice of a longer rowptr ranks a block of
 *   rows against the whole col / rank arrays (n_targets = their length); entries of rows that are not listed are left untouched.
 * dev_rank[e] (int32): the number of non-excluded columns c of the row with key(c) > key(target), key = map(score) << 32 | ~column
 *   (descending score, -0.0 == +0.0, equal scores to the lower column, every NaN below every number and by column) — the slot the
 *   target would hold in an unbounded ncf_topk_rows result.  The row's other targets compete like any column; duplicate targets
 *   get the same rank; a target that is excluded or outside [0, cols) gets -1.
 * dev_ranked[r] (int32): the number of non-excluded columns of row r.
 * Both outputs are initialised inside the call by kernels (no memset node) and accumulated with int32 atomics over column tiles:
 *   bit-reproducible, and a captured call gives the same answer on every replay.  Nothing is launched on a refusal.
 * Workspace (the _workspace_bytes queries; 16-byte aligned, never 0): 12 bytes per target entry, fused calls 32; ncf_mlp_rank adds
 *   the first part's layer-1 state as ncf_mlp_topk does.  1 <= cols <= 2^24, rows <= 65536.
 *
 * ncf_rank_rows: ranks the listed columns of an existing (rows, cols) fp32 score matrix (leading dimension ld).  Any number of
 *   targets per row (processed in chunks of ncf_rank_max_targets() = 128).
 * ncf_dot_rank / ncf_mlp_rank: arguments of ncf_dot_topk / ncf_mlp_topk.  The targets' own scores come from ncf_gather_dot /
 *   ncf_score_fused over the (row, target) pairs, the catalogue's from the top-K kernels' scoring code: the same bits, so the result
 *   is ncf_rank_rows' over the pair scorer's score matrix.  max_targets (1 .. 128; 0 or less NCF_EINVAL, above NCF_EUNSUPPORTED)
 *   sizes the kernel's LDS; 1 is the leave-one-out form (target key and counter in registers).  A row with more targets than
 *   max_targets is not truncated silently: its first max_targets entries are ranked, the others get -1 and *dev_overflow_flag
 *   (sticky, when non-NULL) is set.  Limits as the top-K siblings: D <= 256; ncf_mlp_rank_supported() (fp32, an ncf_score_fused
 *   instance, EA and EB multiples of 8); NCF_EUNSUPPORTED otherwise — score and take ncf_rank_rows.
 * ------------------------------------------------------------------------------------------------ */
int ncf_rank_max_targets(void);
size_t ncf_rank_rows_workspace_bytes(int64_t rows, int64_t cols, int64_t n_targets);
int ncf_rank_rows(const float* dev_scores, int64_t rows, int64_t cols, int64_t ld, const int64_t* dev_seen_rowptr,
                  const int32_t* dev_seen_col, const int64_t* dev_tgt_rowptr, const int32_t* dev_tgt_col, int64_t n_targets,
                  int32_t* dev_rank, int32_t* dev_ranked, void* dev_workspace, size_t workspace_bytes, ncf_stream_t stream);
size_t ncf_dot_rank_workspace_bytes(int64_t rows, int64_t cols, int D, int64_t n_targets, int max_targets);
int ncf_dot_rank(const float* dev_tabA, int64_t rowsA, int64_t ldA, const float* dev_tabB, int64_t rowsB, int64_t ldB,
                 const int64_t* dev_idxA, const int64_t* dev_idxB, int64_t rows, int64_t cols, int D, const int64_t* dev_seen_rowptr,
                 const int32_t* dev_seen_col, const int64_t* dev_tgt_rowptr, const int32_t* dev_tgt_col, int64_t n_targets,
                 int max_targets, int32_t* dev_rank, int32_t* dev_ranked, void* dev_workspace, size_t workspace_bytes,
                 int32_t* dev_oob_flag, int32_t* dev_overflow_flag, ncf_stream_t stream);
int ncf_mlp_rank_supported(int dtype, int EA, int EB, int n_layers, const int* dims, int max_targets);
size_t ncf_mlp_rank_workspace_bytes(int64_t rows, int64_t cols, int user_first, int n_layers, const int* dims, int64_t n_targets,
                                    int max_targets);
int ncf_mlp_rank(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, const void* dev_tabB, int64_t rowsB, int64_t ldB,
                 int EA, int EB, int user_first, const int64_t* dev_user_ids, const int64_t* dev_item_ids, int64_t rows,
                 int64_t cols, int n_layers, const int* dims, const void* dev_packed, const int64_t* dev_seen_rowptr,
                 const int32_t* dev_seen_col, const int64_t* dev_tgt_rowptr, const int32_t* dev_tgt_col, int64_t n_targets,
                 int max_targets, int32_t* dev_rank, int32_t* dev_ranked, void* dev_workspace, size_t workspace_bytes,
                 int32_t* dev_oob_flag, int32_t* dev_overflow_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ncf_ranking_plan — the launch shape one of the six ranking entry points above picks for (rows, cols) and its k (top-K entries)
 * or max_targets (rank entries; ignored by NCF_RANKING_RANK_ROWS), answered on the host without launching and without touching the
 * device (like ncf_linear_plan), by the functions the entry point's own launch calls.  Any output pointer may be NULL.
 *   *tile_cols     columns per workgroup tile (8192 for the score-matrix entries; 2048 / 4096 / 8192 for the dot entries) or per
 *                  wave range (32 .. 8192 for the MLP entries; ncf_mlp_rank with max_targets > 1 stays at 512 or above)
 *   *tiles         ceil(cols / *tile_cols): tiles (ranges) per row
 *   *merge_levels  merge launches after the first level of a top-K entry (0: the first level finishes alone); 0 for a rank entry
 *   *chunk_rows    rows per pass of a top-K entry over its key workspace (== rows: one pass; ncf_dot_topk rounds a partial chunk
 *                  of more than 64 rows down to a multiple of 64); rows for a rank entry
 * Refusals: those the entry point makes on k / max_targets, rows and cols, with its codes; an unknown entry is NCF_EINVAL.  The
 * embedding width, the MLP instance and the exclusion / target lists do not enter a plan.
 * ------------------------------------------------------------------------------------------------ */
enum ncf_ranking_entry {
    NCF_RANKING_TOPK_ROWS = 0, NCF_RANKING_RANK_ROWS = 1, NCF_RANKING_DOT_TOPK = 2, NCF_RANKING_DOT_RANK = 3,
    NCF_RANKING_MLP_TOPK = 4, NCF_RANKING_MLP_RANK = 5
};
int ncf_ranking_plan(int entry, int64_t rows, int64_t cols, int k_or_max_targets, int* tile_cols, int64_t* tiles, int* merge_levels,
                     int64_t* chunk_rows);

/* ------------------------------------------------------------------------------------------------
 * NeuMF (csrc/neumf.hip, csrc/gmf.h; fp32 only) — the fused model of He et al. 2017: an MLP tower over cat(user row, item row) and a
 * GMF branch over a second pair of tables, under one 1-wide output layer `predict` over cat(p (.) q, phi).  Replaces: nothing in the
 * reference, which has the two towers only as separate models.
 * Operands: dev_tabA / dev_tabB are the tower's user / item tables (EA / EB wide), dev_gmfA / dev_gmfB the GMF tables of the same
 *   users / items (D wide, leading dimensions ldGA / ldGB, as many rows as their side's tower table: rowsA / rowsB).
 *   dev_packed = ncf_mlp_pack of [W1, (W2,) predict.weight[:, D:]] and [b1, (b2,) predict.bias] (n_layers, dims as there: dims[0] =
 *   EA + EB, dims[n_layers] = 1);  dev_w = predict.weight[0, :D] (D floats, 16-byte aligned).
 *   D is a multiple of 8 with 8 <= D <= 128.
 * THE CONTRACT, per pair (u, i) with GMF rows p = gmfA[u], q = gmfB[i]:
 *   s_mlp   the bits of the fused scorer's last sum: what ncf_score_fused returns for the pair with the same blob and a zero last
 *           bias.  Layer 1 starts from b1 and runs its k-steps q ascending (the user table's, then the item table's), tiles
 *           nt-major, j ascending; layer 2 and the last sum are the fused scorer's own code.
 *   g       for lane half h in {0, 1} start a_h = +0.f; then for s = 0 .. D/8 - 1 and j = 0 .. 3, with d = 8 s + 4 h + j:
 *               t = fl(w[d] * p[d]);   v = fl(t * q[d]);   a_h = fl(a_h + v)
 *           and g = fl(a_0 + a_1).  Every product and sum is rounded on its own (no FMA).
 *   score = fl(fl(s_mlp + g) + bl[0])        bl = predict.bias
 *   An out-of-range user (item) id reads zero rows in both of that side's tables and sets *dev_oob_flag (when non-NULL).
 *   s_mlp is never -0.0 (see ncf_mlp_topk) and a_h starts at +0, so g is never -0.0 and the score is -0.0 only if fl(s_mlp + g) and
 *   bl both are: the ranking entries below recover the caller's bits from their keys for every non-NaN score.
 * ncf_neumf_supported: dtype NCF_F32, a (K0 = EA + EB, dims) shape with an ncf_score_fused instance, EA and EB both >= 8 and
 *   multiples of 8, D as above.  Every entry returns NCF_EUNSUPPORTED otherwise and launches nothing.
 * ncf_neumf_score: dev_out[b] = score(dev_idxU[b], dev_idxI[b]) for b < B (an id list may be NULL: position b).  One wave per
 *   32-pair tile, one launch form at every B, no host synchronisation: the call captures into a HIP graph.  Tables 16-byte aligned
 *   with ld % 4 == 0 (NCF_EINVAL otherwise).
 * ncf_neumf_topk / ncf_neumf_rank: ncf_mlp_topk / ncf_mlp_rank over NeuMF's score, users first (user_first is not an argument):
 *   exactly ncf_topk_rows / ncf_rank_rows over the matrix of ncf_neumf_score's scores, bit for bit, without that matrix.  Same
 *   output layout, limits (k <= 128, cols <= 2^24, rows <= 65536, max_targets <= 128), exclusion CSR, target CSR and overflow flag
 *   as the MLP entries, and the same waves: the column ranges, merge plan and row chunks are theirs, so
 *   ncf_ranking_plan(NCF_RANKING_MLP_TOPK / NCF_RANKING_MLP_RANK, ...) answers for these two entries as well.  The workspace
 *   (ncf_neumf_topk_workspace_bytes / ncf_neumf_rank_workspace_bytes) is the MLP entry's plus D floats per listed user: the rounded
 *   row t = w (.) p_u, written once per call behind the layer-1 state.
 * ------------------------------------------------------------------------------------------------ */
int ncf_neumf_supported(int dtype, int EA, int EB, int D, int n_layers, const int* dims);
int ncf_neumf_score(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, const void* dev_tabB, int64_t rowsB, int64_t ldB,
                    const float* dev_gmfA, int64_t ldGA, const float* dev_gmfB, int64_t ldGB, const int64_t* dev_idxU,
                    const int64_t* dev_idxI, int64_t B, int EA, int EB, int D, int n_layers, const int* dims, const void* dev_packed,
                    const float* dev_w, float* dev_out, int32_t* dev_oob_flag, ncf_stream_t stream);
size_t ncf_neumf_topk_workspace_bytes(int64_t rows, int64_t cols, int n_layers, const int* dims, int D, int k);
int ncf_neumf_topk(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, const void* dev_tabB, int64_t rowsB, int64_t ldB,
                   const float* dev_gmfA, int64_t ldGA, const float* dev_gmfB, int64_t ldGB, int EA, int EB, int D,
                   const int64_t* dev_user_ids, const int64_t* dev_item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims,
                   const void* dev_packed, const float* dev_w, const int64_t* dev_seen_rowptr, const int32_t* dev_seen_col, int k,
                   float* dev_out_score, int32_t* dev_out_idx, int32_t* dev_out_count, void* dev_workspace, size_t workspace_bytes,
                   int32_t* dev_oob_flag, ncf_stream_t stream);
size_t ncf_neumf_rank_workspace_bytes(int64_t rows, int64_t cols, int n_layers, const int* dims, int D, int64_t n_targets,
                                      int max_targets);
int ncf_neumf_rank(int dtype, const void* dev_tabA, int64_t rowsA, int64_t ldA, const void* dev_tabB, int64_t rowsB, int64_t ldB,
                   const float* dev_gmfA, int64_t ldGA, const float* dev_gmfB, int64_t ldGB, int EA, int EB, int D,
                   const int64_t* dev_user_ids, const int64_t* dev_item_ids, int64_t rows, int64_t cols, int n_layers, const int* dims,
                   const void* dev_packed, const float* dev_w, const int64_t* dev_seen_rowptr, const int32_t* dev_seen_col,
                   const int64_t* dev_tgt_rowptr, const int32_t* dev_tgt_col, int64_t n_targets, int max_targets, int32_t* dev_rank,
                   int32_t* dev_ranked, void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, int32_t* dev_overflow_flag,
                   ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Full-catalogue softmax cross-entropy for a dot-product readout, without a rows x cols matrix (csrc/dot_softmax.hip; fp32 only).
 * Operands as ncf_dot_topk: listed row b is dev_tabA[dev_idxA[b]] (dev_tabA[b] with dev_idxA NULL), catalogue column j is
 * dev_tabB[dev_idxB[j]] (dev_tabB[j] with dev_idxB NULL), D = 1 .. 256, rows <= 65536, cols <= 2^24.
 *   s_bj = <row b, column j>   bit-identical to ncf_gather_dot's fp32 kernel for that pair
 *   z_bj = s_bj * scale        one rounded fp32 product; scale finite and > 0
 * ncf_dot_lse:  dev_lse[b] = m_b + log sum_j exp(z_bj - m_b), m_b = max_j z_bj (exact; written to dev_max when it is not NULL).
 *   The loss of row b with target column t is dev_lse[b] - z_bt.
 * ncf_dot_softmax_grad:  with w_bj = g_b * scale * (exp(z_bj - lse_b) - [j == t_b]), g_b the upstream gradient of row b's loss,
 *   items == 0:  dev_out (rows, D) contiguous, row b = sum_j w_bj * column j      (one row per LISTED row: repeated ids stay apart)
 *   items != 0:  dev_out (cols, D) contiguous, row j = sum_b w_bj * row b
 *   dev_targets (rows) int64 columns in [0, cols), dev_lse / dev_g (rows) fp32.
 * Determinism: no float atomics; a walk that is split into tiles is merged in ascending tile order, so two calls on the same
 * inputs give the same bits.  exp / log are the device library's: results are held to float64 at a tolerance, not bit for bit.
 * Out-of-range ids: an id of dev_idxA / dev_idxB outside its table, or a target outside [0, cols), sets *dev_oob_flag; such a
 * listed row gets a zero gradient row and adds nothing to the columns' (its lse is that of a zero row), such a column is in no
 * denominator and gets a zero gradient row.  Nothing is read or written out of bounds.
 * Workspace (16-byte aligned, >= the query; never grows with rows x cols): ncf_dot_lse keeps 8 bytes per (row, column tile);
 * ncf_dot_softmax_grad keeps tiles x chunk_rows x D floats only when its walk is split (<= 32 MiB, rows taken in chunks).
 * ncf_dot_softmax_plan answers, without launching, the walk tile, the number of tiles and the rows per chunk of
 * kind = NCF_DOT_SOFTMAX_LSE / _GRAD_ROWS (items == 0) / _GRAD_ITEMS (items != 0); any output pointer may be NULL.
 * Refusals: NCF_EUNSUPPORTED for D, rows or cols outside the ranges; NCF_EINVAL for a NULL argument, a leading dimension < D,
 * rows > rowsA without dev_idxA (cols > rowsB without dev_idxB), a scale that is not finite and > 0, an unknown kind;
 * NCF_EWORKSPACE for a short workspace.  rows == 0 returns NCF_OK and launches nothing.
 * ------------------------------------------------------------------------------------------------ */
enum ncf_dot_softmax_kind { NCF_DOT_SOFTMAX_LSE = 0, NCF_DOT_SOFTMAX_GRAD_ROWS = 1, NCF_DOT_SOFTMAX_GRAD_ITEMS = 2 };
int ncf_dot_softmax_plan(int kind, int64_t rows, int64_t cols, int D, int64_t* tile, int64_t* tiles, int64_t* chunk_rows);
size_t ncf_dot_lse_workspace_bytes(int64_t rows, int64_t cols, int D);
int ncf_dot_lse(const float* dev_tabA, int64_t rowsA, int64_t ldA, const float* dev_tabB, int64_t rowsB, int64_t ldB,
                const int64_t* dev_idxA, const int64_t* dev_idxB, int64_t rows, int64_t cols, int D, float scale, float* dev_lse,
                float* dev_max, void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);
size_t ncf_dot_softmax_grad_workspace_bytes(int64_t rows, int64_t cols, int D, int items);
int ncf_dot_softmax_grad(const float* dev_tabA, int64_t rowsA, int64_t ldA, const float* dev_tabB, int64_t rowsB, int64_t ldB,
                         const int64_t* dev_idxA, const int64_t* dev_idxB, int64_t rows, int64_t cols, int D,
                         const int64_t* dev_targets, const float* dev_lse, const float* dev_g, float scale, int items, float* dev_out,
                         void* dev_workspace, size_t workspace_bytes, int32_t* dev_oob_flag, ncf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Calibration probe — the bf16 MFMA rate the chip SUSTAINS on random operands (it lowers its clock under matrix load), so that
 * bench.py can state a kernel's fraction of it next to the fraction of the 2.5 PFLOP/s datasheet figure.  Not part of scoring.
 * Launches `blocks` 512-thread workgroups; every wave issues iters * 32 v_mfma_f32_16x16x32_bf16 (16 384 flop each) on register
 * operands taken from dev_rnd (64 KiB of random bf16 bit patterns, finite values); with_lds != 0 adds the scoring kernels' LDS
 * operand reads.  dev_sink: blocks * 512 floats (written, never meaningful); dev_clk: blocks * 8 pairs of u64
 * {shader cycles, 100 MHz ticks} per wave.  flop per launch = blocks * 8 * iters * 32 * 16384.
 * ------------------------------------------------------------------------------------------------ */
int ncf_probe_mfma_bf16(const void* dev_rnd, int iters, int blocks, int with_lds, float* dev_sink, unsigned long long* dev_clk,
                        ncf_stream_t stream);
/* Memory-side probes for the standalone gather's roofline: a streaming 16-byte copy of `bytes` (the chip's copy ceiling), and
 * random whole-row READS (rows of row_bytes = 16 .. 1024, a power of two; ids from dev_idx, n of them; `inflight` = 1 / 2 / 4 / 8
 * independent rows per lane group; nothing is written but one word per thread into dev_sink (blocks * 256 words)). */
int ncf_probe_copy(const void* dev_src, void* dev_dst, int64_t bytes, ncf_stream_t stream);
int ncf_probe_gather_read(const void* dev_table, int64_t rows, int64_t ld_bytes, int row_bytes, const int64_t* dev_idx, int64_t n,
                          int inflight, int blocks, uint32_t* dev_sink, ncf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NCF_ABI_H */
