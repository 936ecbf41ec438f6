"""Dev tool (GPU box): the measurements of DESIGN §4.21 — pair-wise (BPR) training with negatives drawn on the device.

    python tools/bpr_rate.py [part ...]        parts: sample, cdf, step, epoch (default: all)

  sample  ncf_sample_negatives, 65 536 picks over a CSR of 262 144 rows x 300 negatives (HIP events, back to back)
  cdf     ncf_negative_cdf over 1e8 entries (rows of 300), bytes read + written against a live ncf_probe_copy of the same volume
  step    BasicNCF at the cfg-2 training shape (1 M users x 100 k items, 64/64, MLP [256, 128], batch 65 536, FusedAdam): the
          pair-wise step (gather + sample_negatives + two forwards + BPR + backward + Adam) against the point-wise step at the same
          batch, and the sampling + batch assembly alone
  epoch   train_model, one epoch on the same synthetic ranking file: device-resident loop against the DataLoader loop
"""
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprecommendation_amd import native  # noqa: E402
from deeprecommendation_amd.content_providers.index_providers import IndexProvider  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import NegativeSampler  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.datasets.fixed_datasets import FixedPointwiseDataset, FixedRankingDataset  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.train import train_model  # noqa: E402
from deeprecommendation_amd.optim import FusedAdam  # noqa: E402


def events_us(fn, reps, settle=5):
    for _ in range(settle):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def csr(rows, per_row, dev, seed=0):
    rng = np.random.default_rng(seed)
    rowptr = torch.arange(0, (rows + 1) * per_row, per_row, dtype=torch.int64, device=dev)
    rating = torch.from_numpy((rng.integers(1, 11, rows * per_row) * 0.5).astype(np.float32)).to(dev)
    neg = torch.from_numpy(rng.integers(0, 100_000, rows * per_row).astype(np.int32)).to(dev)
    return rowptr, rating, neg


def part_sample(dev):
    rowptr, rating, neg = csr(262_144, 300, dev)
    cdf = native.negative_cdf(rowptr, rating, 1.5)
    pick = torch.randint(0, 262_144, (65_536,), device=dev)
    out = torch.empty(65_536, dtype=torch.int64, device=dev)
    slot = [0]

    def call():
        native.sample_negatives(rowptr, cdf, neg, pick, 12345, slot[0], out=out)
        slot[0] += 65_536

    us = events_us(call, 200)
    native.check_oob(dev)
    print(f"sample_negatives: 65 536 picks x 300 negatives: {us:.1f} us per call (back to back)", flush=True)


def part_cdf(dev):
    n_rows = 333_334
    rowptr, rating, _ = csr(n_rows, 300, dev)
    cdf = torch.empty_like(rating)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = [0.5, 1.0, 1.5, 3.0]
    k = [0]

    def call():
        native.negative_cdf(rowptr, rating, ws[k[0] % 4], out=cdf, flag=flag)
        k[0] += 1

    us = events_us(call, 20, settle=3)
    nbytes = rating.numel() * 8 + rowptr.numel() * 8            # ratings read + CDF written + rowptr
    src = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = native.load_library()
    copy_us = events_us(lambda: native._check(lib.ncf_probe_copy(src.data_ptr(), dst.data_ptr(), src.numel(), st)), 20, settle=3)
    assert int(flag.item()) == 0
    print(f"negative_cdf: {rating.numel() / 1e6:.0f} M entries in {us:.0f} us = {nbytes / us / 1e3:.0f} GB/s read + written; "
          f"live copy ceiling {2 * src.numel() / copy_us / 1e3:.0f} GB/s: {(nbytes / us) / (2 * src.numel() / copy_us):.2f} of it", flush=True)


def part_step(dev):
    U, I, B = 1_000_000, 100_000, 65_536
    torch.manual_seed(0)
    model = BasicNCF(item_dim=I, user_dim=U, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128]).to(dev).train()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    n = 4 * B
    users = torch.randint(0, U, (n,), device=dev)
    items = torch.randint(0, I, (n,), device=dev)
    y = torch.rand(n, device=dev) * 5
    rowptr, rating, neg = csr(n, 50, dev)
    from deeprecommendation_amd.neural_collaborative_filtering.datasets.base import ResidentPairs

    class _W:
        w = 1.5

    pairs = ResidentPairs(_W, users, items, NegativeSampler(rowptr, neg, rating))
    order = torch.randperm(n, device=dev)
    s = [0]

    def pick():
        p = order[(s[0] % 4) * B:(s[0] % 4 + 1) * B]
        s[0] += 1
        return p

    def pointwise():
        p = pick()
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(model(users[p], items[p]), y[p].view(-1, 1), reduction="sum")
        loss.backward()
        opt.step()

    def pairwise():
        u, i, j = pairs.batch(pick(), 7, s[0] * B)
        opt.zero_grad()
        loss = torch.sum(-torch.log(torch.sigmoid(model(u, i) - model(u, j))))
        loss.backward()
        opt.step()

    def assembly():
        pairs.batch(pick(), 7, s[0] * B)

    res = {}
    for _ in range(2):                                           # alternate, twice: box noise shows in the spread
        for name, fn in (("point-wise", pointwise), ("pair-wise", pairwise), ("assembly", assembly)):
            res.setdefault(name, []).append(events_us(fn, 20, settle=3))
    pairs.check()
    pw, pp, asm = (min(res[k]) for k in ("point-wise", "pair-wise", "assembly"))
    print(f"cfg-2 step, batch 65 536: point-wise {pw:.0f} us, pair-wise {pp:.0f} us ({pp / pw:.2f}x); gather + sample_negatives "
          f"{asm:.1f} us = {100 * asm / pp:.1f} % of the pair-wise step  (all runs: {res})", flush=True)


def part_epoch(dev):
    U, I, n, per_row = 100_000, 20_000, 65_536, 50
    rng = np.random.default_rng(1)
    frame = pd.DataFrame({"userId": rng.integers(1, U + 1, n), "positive_movieId": rng.integers(1, I + 1, n),
                          "negative_movieIds": list(rng.integers(1, I + 1, (n, per_row))),
                          "negative_ratings": list(rng.integers(1, 10, (n, per_row)) * 0.5)})
    val = pd.DataFrame({"userId": rng.integers(1, U + 1, 8192), "movieId": rng.integers(1, I + 1, 8192),
                        "rating": rng.integers(1, 11, 8192) * 0.5})
    prov = IndexProvider(np.arange(1, U + 1), np.arange(1, I + 1))
    tmp = tempfile.mkdtemp()
    for resident in (True, False, True):
        torch.manual_seed(0)
        model = BasicNCF(item_dim=I, user_dim=U, item_emb=64, user_emb=64, mlp_dense_layers=[256, 128])
        ds = FixedRankingDataset(frame, prov)
        marks = []

        class Clock:
            def log(self, d):
                if "epoch" in d:
                    torch.cuda.synchronize()
                    marks.append(time.perf_counter())

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_model(model, ds, FixedPointwiseDataset(val, prov), lr=1e-3, weight_decay=0.0, batch_size=4096, val_batch_size=8192,
                    early_stop=False, final_model_path=None, checkpoint_model_path=os.path.join(tmp, "c.pt"), max_epochs=2, device=dev,
                    resident=resident, verbose=False, wandb=Clock())
        per_epoch = np.diff([t0] + marks)
        print(f"ranking epoch, {n} samples x {per_row} negatives, batch 4096, {'resident' if resident else 'DataLoader'}: "
              f"{', '.join(f'{t * 1e3:.0f} ms' for t in per_epoch)} (train + validation on 8192)", flush=True)


def main():
    dev = torch.device("cuda:0")
    parts = sys.argv[1:] or ["sample", "cdf", "step", "epoch"]
    for p in parts:
        {"sample": part_sample, "cdf": part_cdf, "step": part_step, "epoch": part_epoch}[p](dev)


if __name__ == "__main__":
    main()
