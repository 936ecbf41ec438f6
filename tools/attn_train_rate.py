"""Dev tool (GPU box): the measurements of DESIGN §4.24 and §4.29 — an AttentionNCF training epoch on device-built batches against the
DataLoader loop, at the cfg 3 shape (100 k-item catalogue of 2094 features, batches of 4096 pairs from 64
users with 256 rated items each, item_emb = user_emb = 64, att_dense = 128, MLP [256, 128]).

    python tools/attn_train_rate.py [--scale S] [--rounds N] [part ...]        parts: epoch, split, forms (default: these three), msgdrop

  epoch   train_model, both dynamic datasets, resident=False and resident=True alternating in one process, N rounds of 2 epochs
          each after one untimed round; the SECOND epoch of a call is the figure (host clock, device synchronised at both ends;
          training + validation on 64 samples), reported per step with the spread over the rounds
  split   the resident step in parts (HIP events, back to back, FusedAdam): batch assembly (gathers; + sample_negatives for
          pairs), native.pair_rows alone at the step's shape, forward + loss + backward, the optimiser
  forms   the pair-wise step as one forward of 2B pairs against two forwards of B
  msgdrop the resident step (HIP events, FusedAdam) of three models with equal weights, alternating in one process, N rounds:
          (a) message_dropout = 0.2 with AttentionNCF.message_dropout_on_device (ncf_attn_forward_train / _backward_train),
          (b) the same model without the opt-in: the torch ops of _forward_train (a dense (B, I) score matrix and an isclose over
              B x I x IE elements: point-wise only, and only where that can fit the free device memory; where the isclose still
              runs out of memory the model warns and the step goes on WITHOUT the target mask, as the reference does — counted),
          (c) message_dropout = None on the HIP blocks

--scale S divides the catalogue and the batch by S (a rehearsal of the host side; figures at S > 1 measure overheads).
A training file is 8 batches; it is laid out so that, unshuffled, a batch holds 64 users, as cfg 3's batches do.
"""
import argparse
import contextlib
import io
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
from deeprecommendation_amd.content_providers.index_providers import SparseDynamicProvider  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.datasets.dynamic_datasets import (DynamicPointwiseDataset,  # noqa: E402
                                                                                             DynamicRankingDataset, _dev)
from deeprecommendation_amd.neural_collaborative_filtering.models.attention_ncf import AttentionNCF  # noqa: E402
from deeprecommendation_amd.neural_collaborative_filtering.train import train_model  # noqa: E402
from deeprecommendation_amd.optim import FusedAdam  # noqa: E402

CFG3_DIMS = (100_000, 4096, 256, 2094, 64, 64, 128)    # I, B, nnz, F, IE, UE, A: cfg 3 as bench.py sets it up (bench_extra.CFG3_DIMS)
N_BATCHES, USERS_PER_BATCH = 8, 64


def events_us(fn, reps, settle=3):
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


def workload(scale):
    """(provider, point-wise frame, ranking frame, validation frame, dims)."""
    I, B, nnz, Fdim, IE, UE, A = CFG3_DIMS
    I, B = max(I // scale, 2 * nnz), max(B // scale // USERS_PER_BATCH, 1) * USERS_PER_BATCH
    rng = np.random.default_rng(7)
    feats = (rng.random((I, Fdim), dtype=np.float32) < 0.02).astype(np.float32)
    n_users = N_BATCHES * USERS_PER_BATCH
    users = np.arange(1, n_users + 1)
    rated = [np.sort(rng.choice(I, nnz, replace=False)) + 1 for _ in users]
    ratings = [rng.integers(1, 11, nnz) * 0.5 for _ in users]
    prov = SparseDynamicProvider(np.arange(1, I + 1), feats, users, rated, ratings, [float(r.mean()) for r in ratings])
    per_user = B // USERS_PER_BATCH
    pu, pi, pr, rk = [], [], [], []
    for blk in range(N_BATCHES):                                   # one batch = one block of 64 users, samples in random order
        us = np.repeat(users[blk * USERS_PER_BATCH:(blk + 1) * USERS_PER_BATCH], per_user)
        rng.shuffle(us)
        for u in us:
            k = rng.integers(0, nnz)                               # a candidate the user rated: the target mask acts
            pu.append(u); pi.append(int(rated[u - 1][k])); pr.append(float(ratings[u - 1][k]))
            neg = rng.choice(nnz, 20, replace=False)
            rk.append((u, int(rated[u - 1][k]), rated[u - 1][neg].astype(np.int64), np.maximum(ratings[u - 1][neg], 0.5)))
    point = pd.DataFrame({"userId": pu, "movieId": pi, "rating": pr})
    ranking = pd.DataFrame(rk, columns=["userId", "positive_movieId", "negative_movieIds", "negative_ratings"])
    return prov, point, ranking, point.iloc[:64].reset_index(drop=True), (I, B, nnz, Fdim, IE, UE, A)


def new_model(dims, message_dropout=None):
    I, B, nnz, Fdim, IE, UE, A = dims
    torch.manual_seed(7)
    return AttentionNCF(item_dim=Fdim, item_emb=IE, user_emb=UE, att_dense=A, mlp_dense_layers=[256, 128], message_dropout=message_dropout)


def part_epoch(dev, w, rounds):
    prov, point, ranking, val, dims = w
    B = dims[1]
    tmp = tempfile.mkdtemp()
    val_ds = DynamicPointwiseDataset(val, prov)
    times = {}
    for rnd in range(rounds + 1):                                  # round 0 warms every path (uploads, code objects, allocator)
        for name, make in (("point-wise", lambda: DynamicPointwiseDataset(point, prov)), ("pair-wise", lambda: DynamicRankingDataset(ranking, prov))):
            for resident in (False, True):
                marks = []

                class Clock:
                    def log(self, d):
                        if "epoch" in d:
                            torch.cuda.synchronize()
                            marks.append(time.perf_counter())

                np.random.seed(rnd)
                train_model(new_model(dims), make(), val_ds, lr=1e-3, weight_decay=0.0, batch_size=B, val_batch_size=B, early_stop=False,
                            final_model_path=None, checkpoint_model_path=os.path.join(tmp, "c.pt"), max_epochs=2, device=dev,
                            resident=resident, shuffle=False, verbose=False, wandb=Clock())
                if rnd:
                    times.setdefault((name, resident), []).append((marks[1] - marks[0]) / N_BATCHES)
    for name in ("point-wise", "pair-wise"):
        host, res = times[(name, False)], times[(name, True)]
        print(f"{name} epoch, {N_BATCHES} steps of {B} pairs: DataLoader {min(host) * 1e3:.1f} ms per step (all rounds: "
              f"{', '.join(f'{t * 1e3:.1f}' for t in host)}), resident {min(res) * 1e3:.1f} ms per step ({', '.join(f'{t * 1e3:.1f}' for t in res)}): "
              f"{min(host) / min(res):.2f}x", flush=True)


def _resident_makers(dev, w):
    prov, point, ranking, _, dims = w
    B = dims[1]
    pds, rds = DynamicPointwiseDataset(point, prov), DynamicRankingDataset(ranking, prov)
    res = pds.resident_inputs(dev, B)
    held = [t.to(dev) for t in (*res.tensors, res.targets)]
    inputs = res.train_on_chunk(*held[:-1])
    pairs = rds.resident_pairs(dev)
    k = [0]

    def pick():
        s = (k[0] % N_BATCHES) * B
        k[0] += 1
        return s

    def point_batch():
        s = pick()
        return res.train_on_batch(*[t[s:s + B] for t in inputs], held[-1][s:s + B])

    def pair_batch():
        s = pick()
        return pairs.batch(torch.arange(s, s + B, device=dev), 5, k[0] * B)

    return pds, rds, point_batch, pair_batch, pairs


def part_split(dev, w):
    dims = w[4]
    pds, rds, point_batch, pair_batch, pairs = _resident_makers(dev, w)
    for name, ds, make in (("point-wise", pds, point_batch), ("pair-wise", rds, pair_batch)):
        m = new_model(dims).to(dev).train()
        opt = FusedAdam(m.parameters(), lr=1e-3)
        batch = make()

        def model_step():                                          # forward (pair_rows inside) + loss + backward on a batch already built
            opt.zero_grad()
            a, b = type(ds).do_forward(m, batch, dev)
            ds.calculate_loss(a, b).backward()

        def full_step():
            opt.zero_grad()
            a, b = type(ds).do_forward(m, make(), dev)
            ds.calculate_loss(a, b).backward()
            opt.step()

        full_step()
        um = batch[4]
        pairwise = name == "pair-wise"
        n_pairs = um.pair_row.numel() * (2 if pairwise else 1)
        pair_row = torch.cat((um.pair_row, um.pair_row)) if pairwise else um.pair_row.contiguous()
        with torch.no_grad():
            rated_emb = torch.nn.functional.linear(batch[3], m.ItemEmbeddings[0].weight, m.ItemEmbeddings[0].bias)
            cand_emb = rated_emb[torch.cat((batch[2].index, batch[5].index)) if pairwise else batch[2].index].contiguous()

        def pair_rows():
            native.pair_rows(um.rowptr, um.col, um.val, pair_row, n_pairs * um.max_row_len, (cand_emb, rated_emb))

        runs = {}
        for _ in range(2):                                         # alternate, twice: box noise shows in the spread
            for part, fn in (("assembly", make), ("pair_rows", pair_rows), ("model", model_step), ("optimiser", opt.step), ("step", full_step)):
                runs.setdefault(part, []).append(events_us(fn, 10))
        best = {k_: min(v) for k_, v in runs.items()}
        print(f"{name} resident step, {n_pairs} pairs: {best['step'] / 1e3:.2f} ms; batch assembly {best['assembly']:.0f} us, forward + loss + "
              f"backward {best['model'] / 1e3:.2f} ms (pair_rows alone {best['pair_rows']:.0f} us), optimiser {best['optimiser']:.0f} us  "
              f"(all runs: {runs})", flush=True)
    pairs.check()
    native.check_pair_rows(dev)


def part_forms(dev, w):
    dims = w[4]
    _, rds, _, pair_batch, pairs = _resident_makers(dev, w)
    m = new_model(dims).to(dev).train()
    opt = FusedAdam(m.parameters(), lr=1e-3)

    def one():
        opt.zero_grad()
        a, b = DynamicRankingDataset.do_forward(m, pair_batch(), dev)
        rds.calculate_loss(a, b).backward()
        opt.step()

    def two():
        batch = pair_batch()
        opt.zero_grad()
        a = m(batch[2].float().to(dev), batch[3], _dev(batch[4], dev))
        b = m(batch[5].float().to(dev), batch[3], _dev(batch[4], dev))
        rds.calculate_loss(a, b).backward()
        opt.step()

    runs = {}
    for _ in range(3):
        for name, fn in (("one forward of 2B", one), ("two forwards", two)):
            runs.setdefault(name, []).append(events_us(fn, 10))
    a, b = min(runs["one forward of 2B"]), min(runs["two forwards"])
    print(f"pair-wise resident step: one forward of 2B {a / 1e3:.2f} ms, two forwards {b / 1e3:.2f} ms ({b / a:.2f}x)  (all runs: {runs})", flush=True)
    pairs.check()
    native.check_pair_rows(dev)


def part_msgdrop(dev, w, rounds):
    dims = w[4]
    I, B, IE = dims[0], dims[1], dims[4]
    pds, rds, point_batch, pair_batch, pairs = _resident_makers(dev, w)
    for name, ds, make in (("point-wise", pds, point_batch), ("pair-wise", rds, pair_batch)):
        variants = {"a: HIP, message dropout 0.2": (0.2, True), "b: torch ops, message dropout 0.2": (0.2, False), "c: HIP, no message dropout": (None, False)}
        # (b) compares every candidate row with every rated row: a - b, |a - b| (fp32) and the comparison's result over B x I x IE
        need = (2 * 4 + 1) * B * I * IE + 3 * 4 * B * I
        free = torch.cuda.mem_get_info(dev)[0]
        if name == "pair-wise" or need > 0.8 * free:
            print(f"{name}: (b) is not measured: its target mask alone needs {need * (2 if name == 'pair-wise' else 1) / 2 ** 30:.0f} GiB "
                  f"({free / 2 ** 30:.0f} GiB free)", flush=True)
            del variants["b: torch ops, message dropout 0.2"]
        steps = {}
        for tag, (p, on_device) in variants.items():
            m = new_model(dims, p).to(dev).train()
            m.message_dropout_on_device = on_device
            opt = FusedAdam(m.parameters(), lr=1e-3)

            def step(m=m, opt=opt):
                opt.zero_grad()
                a, b = type(ds).do_forward(m, make(), dev)
                ds.calculate_loss(a, b).backward()
                opt.step()

            steps[tag] = step
        runs, said = {}, io.StringIO()
        for _ in range(rounds):
            for tag, fn in steps.items():
                with contextlib.redirect_stderr(said):
                    runs.setdefault(tag, []).append(events_us(fn, 4 if tag.startswith("b") else 10, settle=1 if tag.startswith("b") else 3))
        unmasked = said.getvalue().count("Could not calculate training mask")
        if unmasked:
            print(f"{name}: {unmasked} of {5 * rounds} steps of (b) could not build the target mask and ran without it", flush=True)
        print(f"{name} resident step, message dropout: " + "; ".join(
            f"({tag}) {min(v) / 1e3:.2f} ms (all rounds: {', '.join(f'{t / 1e3:.2f}' for t in v)})" for tag, v in runs.items()), flush=True)
    pairs.check()
    native.check_pair_rows(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("parts", nargs="*", default=["epoch", "split", "forms"])
    args = ap.parse_args()
    w = workload(args.scale)
    print(f"workload: I, B, nnz, F, IE, UE, A = {w[4]}; {len(w[1])} point-wise and {len(w[2])} pair-wise samples", flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    for p in args.parts:
        {"epoch": lambda: part_epoch(dev, w, args.rounds), "split": lambda: part_split(dev, w), "forms": lambda: part_forms(dev, w),
         "msgdrop": lambda: part_msgdrop(dev, w, args.rounds)}[p]()


if __name__ == "__main__":
    main()
