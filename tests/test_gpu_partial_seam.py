"""GPU tests (MI355X) aimed at the seam between the partial scorer's layers and at its ReLUs.  Layer 2 of
ncf_score_fused_partial is its own helper (fused_layer2_sbase: the weight stream addressed from a scalar base); the tests pin what
a change to that seam can break: which blob b2 and the first Wp2 fragments come from, the ReLU of zeros of either sign, subnormals,
inf and NaN, and the ragged ends of a batch.  Same contract as test_gpu_partial_lds.py: the same bits as native.score_fused (on
int32 views: the ReLU turns a NaN accumulator into 0, an inf one can still reach the score) and as the kernel-order C oracle.

Batch sizes, with R = 4 x CUs x 32 pairs (one round): R/2 + 33 (the smallest batch that stays on the partial kernel: 514 tiles on
an MI355X, two dead waves in the last workgroup, a last tile of one pair), R, and 2R (two waves per SIMD, the headline's form).
All 15 instances run at the first size, <8, 256, 128> at all three.  The N2 = 0 instances (no layer 2) and [128, 64] (four waves
per SIMD; the register counts are in DESIGN 4.20) are among the 15.

ReLU inputs: b1 and b2 each hold -0.0, +0.0 and a subnormal; row 1 of both tables is zeros signed so that, for the pair (1, 1),
every product of layer-1 neuron 3 (bias -0.0) is -0 and the neuron stays -0, while neuron 4 (bias +0.0) sums to +0; row 0 of A
holds inf and NaN and is read directly and, times zero, through out-of-range ids.  The C oracle indexes its tables unchecked and
its NaN is the host's, so the first and the last 1024 pairs, which it checks, keep to in-range ids and off row 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS_A, ROWS_B = 900, 400
SUBNORMAL = 1e-41

# every reachable partial instance: EB / 8 in {4, 8, 12, 16}, (N1, N2) of a fused instance at K0 = EA + EB
SHAPES = [(32, 32, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(64, 64, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(32, 96, h) for h in ([256, 128], [256], [128], [128, 64])] + \
         [(128, 128, h) for h in ([256, 128], [256], [128])]
HEAD = (64, 64, [256, 128])


@pytest.fixture(scope="module")
def native(gpu):
    from deeprecommendation_amd import native as n
    n.load_library()
    return n


def _round(gpu):
    return 4 * torch.cuda.get_device_properties(gpu).multi_processor_count * 32


def _mlp(g, dims):
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(len(dims) - 1)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(len(dims) - 1)]
    for b in bs[:-1]:
        b[3], b[4], b[5] = -0.0, 0.0, SUBNORMAL
    return ws, bs


_cases = {}


def _case(native, gpu, EA, EB, hidden, seed=0):
    """Tables, weights, the packed MLP and P of one shape, built once per module."""
    key = (EA, EB, tuple(hidden), seed)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * seed + 7 * EA + EB + len(hidden))
        ta = torch.randn(ROWS_A, EA, generator=g) * 0.5
        tb = torch.randn(ROWS_B, EB, generator=g) * 0.5
        ws, bs = _mlp(g, [EA + EB] + hidden + [1])
        neg, pos = torch.tensor(-0.0), torch.tensor(0.0)
        ta[1] = torch.where(ws[0][3, :EA] > 0, neg, pos)    # w * x = -0 for every k of neuron 3
        tb[1] = torch.where(ws[0][3, EA:] > 0, neg, pos)
        ta[0, 1], ta[0, 2], ta[0, 5] = float("inf"), float("nan"), -float("inf")
        packed = native.PackedMLP([w.to(gpu) for w in ws], [b.to(gpu) for b in bs])
        tag, tbg = ta.to(gpu), tb.to(gpu)
        _cases[key] = (ta, tb, ws, bs, packed, tag, tbg, native.layer1_partial(tag, packed))
    return _cases[key]


def _ids(B, seed):
    """Ids of a batch: the first and last 1024 pairs in range and off row 0 (the C oracle checks them), with the signed-zero rows
    among them; between them out-of-range ids on both sides and direct reads of row 0."""
    g = torch.Generator().manual_seed(seed)
    ia = torch.randint(1, ROWS_A, (B,), generator=g)
    ib = torch.randint(0, ROWS_B, (B,), generator=g)
    for edge in (slice(0, 1024), slice(B - 1024, B)):
        ia[edge][5::64], ib[edge][5::64] = 1, 1      # neuron 3 stays -0, neuron 4 +0
        ia[edge][6::64] = 1                          # the -0 partial sum meets a real row of B
        ib[edge][7::64] = 1
    ia[-1], ib[-1] = 1, 1                            # the one pair of the last tile at R/2 + 33
    mid = slice(1024, B - 1024)
    ia[mid][0::37] = ROWS_A                          # row 0 (inf, NaN) times zero
    ia[mid][1::41] = -2
    ia[mid][2::43] = 0                               # row 0 itself
    ib[mid][3::47] = ROWS_B
    ib[mid][4::53] = -1
    return ia, ib


def _check(native, gpu, EA, EB, hidden, B):
    from oracle import c_oracle
    ta, tb, ws, bs, packed, tag, tbg, P = _case(native, gpu, EA, EB, hidden)
    ia, ib = _ids(B, seed=B + EA + 3 * EB + len(hidden))
    iag, ibg = ia.to(gpu), ib.to(gpu)
    out = native.score_fused_partial(P, tag, iag, tbg, ibg, packed)
    ref = native.score_fused(tag, iag, tbg, ibg, packed)
    native._oob_flag(gpu).zero_()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    sel = torch.cat([torch.arange(1024), torch.arange(B - 1024, B)])
    exp = c_oracle.score_fused_f32(ta, tb, ia[sel], ib[sel], ws, bs)
    assert torch.equal(out.cpu()[sel].view(torch.int32), exp.view(torch.int32))


@pytest.mark.parametrize("EA,EB,hidden", SHAPES)
def test_every_instance_at_the_smallest_partial_batch(native, gpu, EA, EB, hidden):
    assert native.partial_supported(EA, EB, _case(native, gpu, EA, EB, hidden)[4])
    _check(native, gpu, EA, EB, hidden, _round(gpu) // 2 + 33)


@pytest.mark.parametrize("rounds", [1, 2])
def test_headline_instance_at_one_and_two_rounds(native, gpu, rounds):
    _check(native, gpu, *HEAD, rounds * _round(gpu))


def test_two_weight_sets_alternating_without_sync(native, gpu):
    """Two PackedMLPs alternating on one stream with nothing between the twelve launches: a b2 or Wp2 fragment taken from the
    wrong blob would show as the other MLP's scores."""
    B = 2 * _round(gpu)
    EA, EB, hidden = HEAD
    tag, tbg = _case(native, gpu, EA, EB, hidden)[5:7]
    packs = [_case(native, gpu, EA, EB, hidden, seed=s)[4] for s in (0, 1)]
    Ps = [native.layer1_partial(tag, pk) for pk in packs]
    g = torch.Generator().manual_seed(21)
    ia = torch.randint(1, ROWS_A, (B,), generator=g).to(gpu)
    ib = torch.randint(0, ROWS_B, (B,), generator=g).to(gpu)
    refs = [native.score_fused(tag, ia, tbg, ib, pk) for pk in packs]
    assert not torch.equal(refs[0], refs[1])
    outs = [torch.empty(B, 1, device=gpu) for _ in range(12)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        native.score_fused_partial(Ps[k % 2], tag, ia, tbg, ib, packs[k % 2], out=o)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.view(torch.int32), refs[k % 2].view(torch.int32)), k


def test_captured_graph_of_three_launches_replays_twice(native, gpu):
    R = _round(gpu)
    EA, EB, hidden = HEAD
    ta, tb, ws, bs, packed, tag, tbg, P = _case(native, gpu, EA, EB, hidden)
    sizes = [2 * R, R // 2 + 33, R]
    g = torch.Generator().manual_seed(22)
    ids = [(torch.randint(1, ROWS_A, (B,), generator=g).to(gpu), torch.randint(0, ROWS_B, (B,), generator=g).to(gpu)) for B in sizes]
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
            assert torch.equal(o.view(torch.int32), r.view(torch.int32))
