"""GPU: the fused top-K and rank kernels on every launch form the host can pick (tests/rank_forms_ref.py FORMS), each
against the exact vectorised oracle over float64 torch scores of integer data (no sibling kernel): ncf_dot_topk and ncf_dot_rank on
column tiles of 2048, 4096 and 8192 (two and four bitmap rebuilds inside a tile), ncf_dot_topk in row chunks, ncf_mlp_topk and
ncf_mlp_rank on ranges of 32 ... 8192 columns for every fused instance in both concat orders, with and without exclusion lists, on
random rows with heavy ties and on adversarial column orders.  Every comparison is torch.equal on ids, counts, ranks and the int32
view of the scores (NaN compared as NaN); every test first asserts through native.ranking_plan that it runs the form it claims."""
import pytest
import torch

import rank_forms_ref as rf

pytestmark = pytest.mark.gpu


def _assert_form(entry, rows, cols, kt, tile, chunk=None):
    from deeprecommendation_amd import native
    t, tiles, _, ch = native.ranking_plan(entry, rows, cols, kt)
    assert (t, tiles) == (tile, -(-cols // tile)) and ch == (rows if chunk is None else chunk), (entry, rows, cols, kt, t, ch)


def _assert_topk(got, ref):
    torch.cuda.synchronize()
    assert torch.equal(got[2], ref[2])
    assert torch.equal(got[1], ref[1])
    nan = torch.isnan(ref[0])
    assert torch.equal(torch.isnan(got[0]), nan)
    assert torch.equal(got[0][~nan].view(torch.int32), ref[0][~nan].view(torch.int32))


def _assert_rank(got, ref):
    torch.cuda.synchronize()
    assert torch.equal(got[1], ref[1])          # ranked
    assert torch.equal(got[0], ref[0])


def _clean(dev):
    from deeprecommendation_amd import native
    native.check_oob(dev)
    native.check_rank_overflow(dev)


# The parameters of every test come from rf.cases(), the table the CPU test holds to the forms table (FORMS) and to the plans.
def _differ(a, b):
    """The exclusion list changes the expected result (ids or ranks, and the counts of ranked columns)."""
    return not torch.equal(a[1], b[1]) and (len(a) == 3 or not torch.equal(a[0], b[0]))


# ------------------------------------------------------------------------------------------------------------------ dot entries
class _DotCase:
    def __init__(self, tile, kind, D, dev):
        self.tile, self.kind, self.D, self.rows, self.cols = tile, kind, D, rf.DOT_ROWS, rf.form_cols(tile)
        A, B = rf.dot_tables(self.rows, self.cols, tile, D, kind)
        self.a, self.b = rf.dot_float(A, B, kind, dev)
        scores = rf.dot_scores(self.a, self.b)
        plain = rf.Ranking(scores)
        self.seen = {False: None, True: rf.exclusion(self.rows, self.cols, tile, dev, best=plain.topk(2)[1])}
        self.ref = {False: plain, True: rf.Ranking(scores, self.seen[True])}

    def check(self, dev, ids, items=None, item_ids=None, **only):
        """Every k and max_targets rf.cases() lists for this data (only: one entry point, or excl=False or True alone)."""
        from deeprecommendation_amd import native
        items = self.b if items is None else items
        n = 0
        for c in rf.select(tile=self.tile, kind=self.kind, D=self.D, ids=ids, **only):
            kt, excl = c["kt"], c["excl"]
            assert (c["rows"], c["cols"]) == (self.rows, self.cols)
            _assert_form(c["entry"], self.rows, self.cols, kt, self.tile)
            if c["entry"] == "dot_topk":
                _assert_topk(native.dot_topk(self.a, None, items, item_ids, kt, self.seen[excl]), self.ref[excl].topk(kt))
                assert _differ(self.ref[False].topk(kt), self.ref[True].topk(kt))
            else:
                tg = rf.targets(self.rows, self.cols, kt, dev)
                _assert_rank(native.dot_rank(self.a, None, items, item_ids, tg, kt, self.seen[excl]), self.ref[excl].rank(tg))
                assert _differ(self.ref[False].rank(tg), self.ref[True].rank(tg))
            n += 1
        assert n
        _clean(dev)


def test_dot_data_covers_the_dot_cases():
    """The dot tests below run every dot case of rf.cases(): the fixture's data, the id-list data, D = 256 and the chunked pair."""
    data = {(c["tile"], c["kind"], c["D"], c["ids"]) for c in rf.cases() if c["entry"].startswith("dot")}
    assert data == {(t, kind, 16, False) for t, kind in DOT_DATA} | {(4096, "adversarial", 16, True), (8192, "random", 256, False),
                                                                     (8192, "chunked", 4, False)}


DOT_DATA = sorted({(c["tile"], c["kind"]) for c in rf.select(D=16, ids=False)})


@pytest.fixture(scope="module", params=DOT_DATA, ids=lambda p: f"tile{p[0]}-{p[1]}")
def dot_case(request, gpu):
    case = _DotCase(*request.param, 16, gpu)
    yield case
    del case.ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("excl", [False, True], ids=["all", "excl"])
def test_dot_topk_forms(dot_case, excl, gpu):
    """ncf_dot_topk at k = 1, 100 and 128, without and with the exclusion list."""
    dot_case.check(gpu, ids=False, excl=excl, entry="dot_topk")


@pytest.mark.parametrize("excl", [False, True], ids=["all", "excl"])
def test_dot_rank_forms(dot_case, excl, gpu):
    """ncf_dot_rank at max_targets 1 (the register sink), 16 and, on the 8192 form, 128 (the launch with more than 64 KiB of
    dynamic LDS); ranks and ranked; without and with the exclusion list."""
    dot_case.check(gpu, ids=False, excl=excl, entry="dot_rank")


def test_dot_item_id_list_on_the_4096_form(gpu):
    """The ranked list as ids into a longer, shuffled item table: the answer is the plain one's."""
    c = _DotCase(4096, "adversarial", 16, gpu)
    perm = torch.randperm(c.cols + 77, device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    table = torch.full((c.cols + 77, 16), 9.0, device=gpu)
    table[perm[:c.cols]] = c.b
    c.check(gpu, ids=True, items=table, item_ids=perm[:c.cols].contiguous())


def test_dot_width_256_on_the_8192_form(gpu):
    """Four MFMA steps per item block (D = 256) on the 8192 form, random integer rows, with exclusion."""
    _DotCase(8192, "random", 256, gpu).check(gpu, ids=False)


def test_dot_topk_in_row_chunks(gpu):
    """130 users x 2^24 items at k = 128: the key workspace holds 64 rows, so the rows go in chunks of 64, 64 and 2 (a partial chunk
    is rounded down to whole 64-user blocks).  The users differ from chunk to chunk (rf.chunked_case) and the odd rows of every
    chunk exclude their own best columns, so the row offset of a chunk is pinned on the user rows, the exclusion lists and the
    outputs.  The reference is analytic (one stable sort of g in each direction), not a score matrix."""
    from deeprecommendation_amd import native
    without, with_list = rf.select(kind="chunked", excl=False), rf.select(kind="chunked", excl=True)
    assert len(without) == len(with_list) == 1
    c = without[0]
    rows, cols, k = c["rows"], c["cols"], c["kt"]
    _assert_form("dot_topk", rows, cols, k, 8192, chunk=64)
    users, items, seen, ref_plain, ref_excl = rf.chunked_case(rows, cols, k, gpu)
    assert _differ(ref_plain, ref_excl)
    _assert_topk(native.dot_topk(users, None, items, None, k), ref_plain)
    _assert_topk(native.dot_topk(users, None, items, None, k, seen), ref_excl)
    _clean(gpu)


# ------------------------------------------------------------------------------------------------------------------ MLP entries
class _MlpCase:
    def __init__(self, inst, tile, dev):
        self.inst, self.tile, self.rows, self.cols, self.dev = inst, tile, rf.MLP_ROWS, rf.form_cols(tile), dev
        self.m = rf.int_mlp(inst, self.cols, tile, self.rows, seed=sum(inst) + tile)
        self.users, self.items = self.m["users"].float().to(dev), self.m["items"].float().to(dev)
        scores = rf.mlp_scores(self.m, dev)
        plain = rf.Ranking(scores)
        self.seen = {False: None, True: rf.exclusion(self.rows, self.cols, tile, dev, best=plain.topk(2)[1])}
        self.ref = {False: plain, True: rf.Ranking(scores, self.seen[True])}
        self.packed = {}

    def operands(self, user_first):
        from deeprecommendation_amd import native
        if user_first not in self.packed:
            self.packed[user_first] = native.PackedMLP(*rf.mlp_weights(self.m, user_first, self.dev))
        tabs = (self.users, None, self.items, None) if user_first else (self.items, None, self.users, None)
        return tabs + (self.packed[user_first],)


MLP_DATA = sorted({(c["inst"], c["tile"]) for c in rf.cases() if c["entry"].startswith("mlp")},
                  key=lambda p: (p[0] != rf.MAIN, rf.INSTANCES.index(p[0]), p[1]))


def test_mlp_data_covers_the_mlp_cases():
    assert set(MLP_DATA) == {(rf.MAIN, t) for t in rf.MLP_TILES} | {(i, 1024) for i in rf.INSTANCES}


@pytest.fixture(scope="module", params=MLP_DATA, ids=lambda p: "x".join(map(str, p[0])) + f"-tile{p[1]}")
def mlp_case(request, gpu):
    case = _MlpCase(*request.param, gpu)
    yield case
    del case.ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("user_first", [True, False], ids=["user_first", "item_first"])
def test_mlp_topk_forms(mlp_case, user_first, gpu):
    """Instance (128,256,128) on all nine range widths, every other instance at 1024 (wider than 224 columns: the running threshold
    and the in-loop re-select run), k = 100 and one of {1, 10, 100, 128} in turn, without and with the exclusion list."""
    from deeprecommendation_amd import native
    c = mlp_case
    todo = rf.select(entry="mlp_topk", inst=c.inst, tile=c.tile)
    assert {x["excl"] for x in todo} == {False, True}
    for x in todo:
        k, excl = x["kt"], x["excl"]
        assert (x["rows"], x["cols"]) == (c.rows, c.cols)
        _assert_form("mlp_topk", c.rows, c.cols, k, c.tile)
        got = native.mlp_topk(*c.operands(user_first), k, c.seen[excl], user_first=user_first)
        _assert_topk(got, c.ref[excl].topk(k))
        assert _differ(c.ref[False].topk(k), c.ref[True].topk(k))
    _clean(gpu)


@pytest.mark.parametrize("user_first", [True, False], ids=["user_first", "item_first"])
def test_mlp_rank_forms(mlp_case, user_first, gpu):
    """The one-target sink on every range width; the multi-target sink (its floor is 512 columns) with max_targets 3 and 128 on
    instance (128,256,128) and 16 on the others; ranks and ranked, without and with the exclusion list."""
    from deeprecommendation_amd import native
    c = mlp_case
    todo = rf.select(entry="mlp_rank", inst=c.inst, tile=c.tile)
    assert {x["excl"] for x in todo} == {False, True} and 1 in {x["kt"] for x in todo}
    for x in todo:
        mt, excl = x["kt"], x["excl"]
        _assert_form("mlp_rank", c.rows, c.cols, mt, c.tile)
        tg = rf.targets(c.rows, c.cols, mt, gpu)
        got = native.mlp_rank(*c.operands(user_first), tg, mt, c.seen[excl], user_first=user_first)
        _assert_rank(got, c.ref[excl].rank(tg))
        assert _differ(c.ref[False].rank(tg), c.ref[True].rank(tg))
    _clean(gpu)
