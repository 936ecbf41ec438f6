"""GPU tests (MI355X) of the partial scorer's LDS form: the instances of ncf_score_fused_partial whose layer-1 weight image
fits a CU's LDS twice read it from there, the others stream it as before.  Same contract as test_gpu_partial_layer1.py:
bit-identity with native.score_fused (torch.equal, on int32 views where a NaN can occur), and with the kernel-order C oracle.
What is new here is what an LDS image adds: a fill shared by four waves, one barrier that dead waves of a ragged last
workgroup must reach too, and an image per launch that back-to-back launches with different weights must not share."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _round(gpu):
    """Pairs in one round of the one-wave-per-tile kernels: 4 waves x CUs tiles of 32 pairs."""
    return 4 * torch.cuda.get_device_properties(gpu).multi_processor_count * 32


def _mlp(g, dims):
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(len(dims) - 1)]
    return ws, bs


def _case(native, gpu, EA, EB, hidden, rowsA=900, rowsB=400, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * EA + EB + len(hidden))
    ta = torch.randn(rowsA, EA, generator=g) * 0.5
    tb = torch.randn(rowsB, EB, generator=g) * 0.5
    ws, bs = _mlp(g, [EA + EB] + hidden + [1])
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    return g, ta, tb, ws, bs, packed


# every reachable partial instance: EB / 8 in {4, 8, 12, 16}, (N1, N2) of a fused instance at K0 = EA + EB
SHAPES = [(32, 32, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(64, 64, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(32, 96, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(128, 128, h) for h in ([256, 128], [256], [128])]


def _expect_lds(EB, hidden):
    return (EB // 8) * (hidden[0] // 32) <= 80   # KiB of image; two workgroups share a CU's 160 KiB


def test_shapes_cover_both_forms():
    assert sum(_expect_lds(EB, h) for _, EB, h in SHAPES) == 11
    assert sum(not _expect_lds(EB, h) for _, EB, h in SHAPES) == 4


@pytest.mark.parametrize("EA,EB,hidden", SHAPES)
def test_every_instance_equals_fused_and_c_oracle(native, gpu, EA, EB, hidden):
    """Each instance, in LDS or streaming as the dispatch decides, at a ragged batch that stays on the partial kernel (one round +
    20 001 pairs: more than half a round of tail, tiles % 4 != 0, B % 32 != 0: dead waves in the last workgroup and a partial last
    tile) and at two full rounds.  The kernel-order C oracle checks the first 1024 and the last 1024 pairs of the ragged batch."""
    from oracle import c_oracle
    g, ta, tb, ws, bs, packed = _case(native, gpu, EA, EB, hidden)
    assert native.partial_supported(EA, EB, packed)
    assert native.partial_in_lds(EA, EB, packed) == _expect_lds(EB, hidden)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    R = _round(gpu)
    for B in (R + 20001, 2 * R):
        ia = torch.randint(0, ta.shape[0], (B,), generator=g)
        ib = torch.randint(0, tb.shape[0], (B,), generator=g)
        out = native.score_fused_partial(P, tag, ia.to(gpu), tbg, ib.to(gpu), packed)
        assert torch.equal(out, native.score_fused(tag, ia.to(gpu), tbg, ib.to(gpu), packed)), B
        if B % 32:
            sel = torch.cat([torch.arange(1024), torch.arange(B - 1024, B)])
            assert torch.equal(out.cpu()[sel], c_oracle.score_fused_f32(ta, tb, ia[sel], ib[sel], ws, bs)), B


@pytest.mark.parametrize("EA,EB,hidden", [(64, 64, [256, 128]), (32, 32, [128, 64]), (128, 128, [128]), (32, 96, [256, 128])])
@pytest.mark.parametrize("rounds_x2,extra", [(2, 0), (2, 20001), (4, 0), (6, 0)])
def test_batch_sizes(native, gpu, EA, EB, hidden, rounds_x2, extra):
    """Exactly one round, one round + 20 001, two and three rounds (32 768, 52 769, 65 536, 98 304 pairs on an MI355X)."""
    B = rounds_x2 * _round(gpu) // 2 + extra
    g, ta, tb, ws, bs, packed = _case(native, gpu, EA, EB, hidden, rowsA=20000, rowsB=5000, seed=B)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, ta.shape[0], (B,), generator=g).to(gpu)
    ib = torch.randint(0, tb.shape[0], (B,), generator=g).to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    assert torch.equal(out, native.score_fused(tag, ia, tbg, ib, packed))


@pytest.mark.parametrize("idA,idB", [(True, True), (True, False), (False, True)])
def test_identity_ids(native, gpu, idA, idB):
    """idxA / idxB = None: pair p reads row p.  No split is possible there, so the ragged batch runs on the partial kernel whole."""
    B = _round(gpu) + 20001
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=B, rowsB=B, seed=3)
    assert native.partial_in_lds(64, 64, packed)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = None if idA else torch.randint(0, B, (B,), generator=g).to(gpu)
    ib = None if idB else torch.randint(0, B, (B,), generator=g).to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed, B=B)
    assert torch.equal(out, native.score_fused(tag, ia, tbg, ib, packed, B=B))


def test_out_of_range_ids_match_fused_and_set_flag(native, gpu):
    B = _round(gpu) + 20001
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=5000, rowsB=3000, seed=5)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, 5000, (B,), generator=g)
    ib = torch.randint(0, 3000, (B,), generator=g)
    ia[::97] = 5000 + torch.arange(ia[::97].numel())
    ia[5::89] = -3
    ib[3::71] = 3000
    ib[7::83] = -1
    ia[-1], ib[-2] = 5000, -7            # in the partial last tile too
    ia, ib = ia.to(gpu), ib.to(gpu)
    native._oob_flag(gpu).zero_()
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    ref = native.score_fused(tag, ia, tbg, ib, packed)
    with pytest.raises(IndexError):
        native.check_oob(gpu)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_in_range_ids_leave_flag_clear_with_dead_waves(native, gpu):
    """The dead waves of the last workgroup run up to the barrier on clamped ids: they must not raise the flag."""
    B = _round(gpu) + 20001              # 626 tiles past the round: two dead waves in the last workgroup
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], seed=6)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, 900, (B,), generator=g).to(gpu)
    ib = torch.randint(0, 400, (B,), generator=g).to(gpu)
    ia[-1], ib[-1] = 899, 399            # the ids the dead waves and the lanes past B are clamped to: the last rows
    native._oob_flag(gpu).zero_()
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    native.check_oob(gpu)                # raises if the flag is set
    assert torch.equal(out, native.score_fused(tag, ia, tbg, ib, packed))


def test_nonfinite_row0_and_negative_zero_bias(native, gpu):
    """Row 0 of A holding inf / NaN (read, times zero, for an out-of-range id) and a -0.0 entry of b1: same bits as score_fused."""
    B = _round(gpu) + 20001
    g = torch.Generator().manual_seed(11)
    ta = torch.randn(4000, 64, generator=g) * 0.5
    tb = torch.randn(2000, 64, generator=g) * 0.5
    ta[0, 3] = float("inf")
    ta[0, 17] = float("nan")
    ta[0, 40] = -float("inf")
    ws, bs = _mlp(g, [128, 256, 128, 1])
    bs[0][5] = -0.0
    bs[0][6] = 0.0
    packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.randint(0, 4000, (B,), generator=g)
    ib = torch.randint(0, 2000, (B,), generator=g)
    ia[::50] = 0
    ia[1::61] = 4000      # out of range: row 0 times zero
    ia, ib = ia.to(gpu), ib.to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    ref = native.score_fused(tag, ia, tbg, ib, packed)
    native._oob_flag(gpu).zero_()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))


def test_all_pairs_name_one_user(native, gpu):
    """Every wave of every workgroup gathers the same P row."""
    B = 2 * _round(gpu)
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=3000, rowsB=5000, seed=8)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    ia = torch.full((B,), 1234, dtype=torch.int64, device=gpu)
    ib = torch.randint(0, 5000, (B,), generator=g).to(gpu)
    out = native.score_fused_partial(P, tag, ia, tbg, ib, packed)
    assert torch.equal(out, native.score_fused(tag, ia, tbg, ib, packed))


def test_two_weight_sets_alternating_without_sync(native, gpu):
    """Two PackedMLPs used alternately on one stream with nothing between the launches: each launch fills its own LDS image, so a
    stale or racing fill would show as the other MLP's scores."""
    B = 2 * _round(gpu)
    g, ta, tb, ws, bs, packed0 = _case(native, gpu, 64, 64, [256, 128], rowsA=20000, rowsB=5000, seed=9)
    ws1, bs1 = _mlp(g, [128, 256, 128, 1])
    packed1 = native.PackedMLP([w.to(gpu) for w in ws1], [b.to(gpu) for b in bs1])
    tag, tbg = ta.to(gpu), tb.to(gpu)
    Ps = [native.layer1_partial(tag, packed0), native.layer1_partial(tag, packed1)]
    packs = [packed0, packed1]
    ia = torch.randint(0, 20000, (B,), generator=g).to(gpu)
    ib = torch.randint(0, 5000, (B,), generator=g).to(gpu)
    refs = [native.score_fused(tag, ia, tbg, ib, pk) for pk in packs]
    assert not torch.equal(refs[0], refs[1])
    outs = [torch.empty(B, 1, device=gpu) for _ in range(12)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        native.score_fused_partial(Ps[k % 2], tag, ia, tbg, ib, packs[k % 2], out=o)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o, refs[k % 2]), k


def test_captured_graph_of_several_launches_replays(native, gpu):
    R = _round(gpu)
    g, ta, tb, ws, bs, packed = _case(native, gpu, 64, 64, [256, 128], rowsA=20000, rowsB=5000, seed=10)
    tag, tbg = ta.to(gpu), tb.to(gpu)
    P = native.layer1_partial(tag, packed)
    sizes = [2 * R, R + 20001, R]
    ids = [(torch.randint(0, 20000, (B,), generator=g).to(gpu), torch.randint(0, 5000, (B,), generator=g).to(gpu)) for B in sizes]
    refs = [native.score_fused(tag, ia, tbg, ib, packed) for ia, ib in ids]
    outs = [torch.empty(B, 1, device=gpu) for B in sizes]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for (ia, ib), o in zip(ids, outs):
            native.score_fused_partial(P, tag, ia, tbg, ib, packed, out=o)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for (ia, ib), o in zip(ids, outs):
            native.score_fused_partial(P, tag, ia, tbg, ib, packed, out=o)
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        for o, r in zip(outs, refs):
            assert torch.equal(o, r)
