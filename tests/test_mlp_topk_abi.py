"""CPU: the fused MLP top-K (ncf_mlp_topk) is declared in the C ABI, exported by the built library and bound in Python; its host-side
shape queries answer without a GPU."""
import os
import re

from conftest import ROOT

NAMES = ("ncf_mlp_topk", "ncf_mlp_topk_workspace_bytes", "ncf_mlp_topk_supported")


def _lib():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load_library()


def test_header_declares_mlp_topk():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ncf_abi.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", txt), name


def test_library_exports_and_binding():
    from deeprecommendation_amd import native
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in native.SIGNATURES, name
    assert callable(native.mlp_topk) and callable(native.mlp_topk_supported)
    assert native.MLP_TOPK_MAX_K == 128


def test_supported_query_follows_the_fused_instances():
    from deeprecommendation_amd import native
    lib = _lib()
    d = native._dims_array
    ok = lambda EA, EB, dims, k, dt=native.NCF_F32: bool(lib.ncf_mlp_topk_supported(dt, EA, EB, len(dims) - 1, d(dims), k))
    for K0, N1, N2 in ((64, 256, 128), (64, 256, 0), (64, 128, 0), (64, 128, 64), (128, 256, 128), (128, 256, 0), (128, 128, 0),
                       (128, 128, 64), (256, 256, 128), (256, 256, 0), (256, 128, 0)):
        dims = [K0, N1, N2, 1] if N2 else [K0, N1, 1]
        assert ok(K0 // 2, K0 // 2, dims, 10) and ok(8, K0 - 8, dims, 128) and ok(K0 - 8, 8, dims, 1)
        assert not ok(K0, 0, dims, 10)                          # both parts must be present
        assert not ok(K0 // 2, K0 // 2, dims, 129)              # above the fused limit on k
        assert not ok(K0 // 2, K0 // 2, dims, 10, native.NCF_BF16)
    assert not ok(60, 68, [128, 256, 128, 1], 10)                # split not a multiple of 8
    assert not ok(64, 64, [128, 64, 1], 10)                      # no fused instance
    assert not ok(64, 64, [128, 256, 128, 2], 10)                # last layer not 1 wide


def test_workspace_query():
    from deeprecommendation_amd import native
    lib = _lib()
    dims = native._dims_array([128, 256, 128, 1])
    assert lib.ncf_mlp_topk_workspace_bytes(0, 1000, 1, 3, dims, 10) == 0
    assert lib.ncf_mlp_topk_workspace_bytes(4, 1000, 1, 3, dims, 0) == 0
    assert lib.ncf_mlp_topk_workspace_bytes(4, 1000, 1, 3, dims, 129) == 0
    u = lib.ncf_mlp_topk_workspace_bytes(4096, 65536, 1, 3, dims, 100)
    i = lib.ncf_mlp_topk_workspace_bytes(4096, 65536, 0, 3, dims, 100)
    assert u > 4096 * 256 * 4 and u % 16 == 0
    assert i - u == (65536 - 4096) * 256 * 4                    # the item-first state is per column, the user-first per row
