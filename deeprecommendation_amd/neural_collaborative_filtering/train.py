"""Training loop of the reference (train.py:21-227: epochs of zero_grad -> do_forward -> loss -> backward -> step, validation
per epoch, checkpoint of the best epoch, patience-based early stopping), with the same arguments and the same returned
``monitored_metrics``; tqdm / W&B output is reduced to optional ``wandb.log`` calls.

Point-wise datasets: MSE (or BCE) loss, validation loss + NDCG, early stopping on the validation loss.  Pair-wise datasets
(``RankingDataset``, train.py:79-210): the negative-sampling exponent ``w`` follows ``schedule_w`` from epoch to epoch, the
loss is BPR, validation gives NDCG only and early stopping watches it (a maximising ``EarlyStopping``).

What differs is how batches reach the GPU.  For datasets whose batch is a pure function of the sample rows
(``Dataset.resident_inputs``: index ids) the whole training file is uploaded ONCE, every epoch draws a permutation on the
device and a batch is a gather of ids — no per-sample ``__getitem__``, no collate, no per-batch host-to-device copy — and
the running loss stays on the GPU (the reference synchronises with ``loss.item()`` and copies ``out`` to the host every
batch, train.py:107-110).  Pair-wise datasets over index ids (``RankingDataset.resident_pairs``) keep the negatives' CSR on
the device too, and a batch's negatives are one ``native.sample_negatives`` call (a per-epoch seed from torch's default
generator, slots numbered across the epoch) instead of the reference's per-sample host draw.  Other datasets run the
reference-shaped ``DataLoader(shuffle=True)`` loop.  The default optimiser on a GPU is ``FusedAdam`` (torch.optim.Adam's
update as one kernel per tensor).
"""
import numpy as np
import torch
from torch import optim
from torch.utils.data import DataLoader

from .. import native
from .datasets.base import PointwiseDataset, RankingDataset
from .eval import eval_model
from .util import cap_host_threads, load_model


class EarlyStopping:
    """The reference's stopping rule (train.py:157-210) as a small state machine over the monitored value.

    * a new overall best: remember it (the caller checkpoints), strikes back to 0, budget back to ``max_patience``;
    * otherwise: one strike if the value also got worse against the PREVIOUS epoch, else one strike is forgiven (never below
      0); the budget shrinks by one regardless; stop when strikes exceed ``patience`` or the budget is used up.
    ``maximize=False`` (point-wise: validation loss) — better is strictly lower; ``maximize=True`` (pair-wise: validation NDCG)
    — better is strictly higher.  NaN compares as the reference's comparisons do (never better, never worse).
    """

    def __init__(self, patience=3, max_patience=5, maximize=False):
        self.patience, self.full_budget, self.maximize = patience, max_patience, maximize
        self.budget, self.strikes = max_patience, 0
        self.best, self.previous, self.best_epoch = None, None, -1

    def update(self, value: float, epoch: int) -> str:
        """'best' (checkpoint now), 'stop', or 'continue'."""
        if self.best is None or (value > self.best if self.maximize else value < self.best):
            self.best, self.best_epoch = value, epoch
            self.strikes, self.budget = 0, self.full_budget
            verdict = "best"
        else:
            if self.previous is not None and (value < self.previous if self.maximize else value > self.previous):
                self.strikes += 1
            else:
                self.strikes = max(0, self.strikes - 1)
            self.budget -= 1
            verdict = "stop" if (self.strikes > self.patience or self.budget <= 0) else "continue"
        self.previous = value
        return verdict


def schedule_w(epoch, break_points=(4, 8, 12, 18, 24)):
    """train.py:229-243: the negative-sampling exponent of an epoch (counted from 1).  The ``2`` branch repeats the condition
    before it and is never taken, as in the reference: the values are 0, 0.5, 1, 1.5, 3."""
    break_points = sorted(break_points)
    assert len(break_points) >= 5, 'Invalid args'
    if epoch < break_points[0]:
        return 0.0
    elif epoch < break_points[1]:
        return 0.5
    elif epoch < break_points[2]:
        return 1
    elif epoch < break_points[3]:
        return 1.5
    elif epoch < break_points[3]:
        return 2
    else:
        return 3


def _resident_training_inputs(dataset, device, batch_size, per_batch_hook=False):
    """(inputs on the device, targets on the device, on_batch or None) for the whole file, or None.  ``on_chunk`` runs once on the
    uploaded file, ``on_batch`` per picked batch (``ResidentInputs.train_on_*``: the forms that survive validation passes).  A
    dataset whose batches need an ``on_batch`` hook is taken only with ``per_batch_hook`` (train_model's ``resident=True``)."""
    if torch.device(device).type != "cuda":
        return None
    res = dataset.resident_inputs(torch.device(device), batch_size)
    if res is None or (res.on_batch is not None and not per_batch_hook):
        return None
    dev = [t.pin_memory().to(device, non_blocking=True) for t in (*res.tensors, res.targets)]
    inputs = list(res.train_on_chunk(*dev[:-1])) if res.train_on_chunk is not None else dev[:-1]
    return inputs, dev[-1], res.train_on_batch


def train_model(model, train_dataset, val_dataset: PointwiseDataset, lr, weight_decay, batch_size, val_batch_size, early_stop,
                final_model_path='final_model.pt', checkpoint_model_path='temp.pt', max_epochs=100, patience=3, max_patience=5,
                optimizer=None, ndcg_cutoff=10, wandb=None, num_workers=0, device=None, resident=None, shuffle=True, verbose=True):
    """train.py:21-227 for point-wise and pair-wise (ranking) training datasets.  Extra keyword arguments: ``device`` (default:
    cuda:0 when there is one), ``resident`` (None = device-resident batches when the dataset allows, False = DataLoader loop,
    True = device-resident batches or ValueError), ``shuffle`` (tests).  The two dynamic datasets (AttentionNCF: ``resident_opt_in``)
    build their batches on the device only with ``resident=True``; ``None`` keeps their DataLoader loop, so no existing run changes."""
    ranking = isinstance(train_dataset, RankingDataset)
    if not (ranking or isinstance(train_dataset, PointwiseDataset)) or not isinstance(val_dataset, PointwiseDataset):
        raise NotImplementedError("train_model takes a point-wise or a ranking (pair-wise) training dataset and a point-wise "
                                  "validation dataset")
    device = torch.device(device) if device is not None else torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    cap_host_threads()
    model.to(device)
    if not model.is_dataset_compatible(train_dataset.__class__) or not model.is_dataset_compatible(val_dataset.__class__):
        raise Exception('Model used is incompatible with this dataset.')
    say = print if verbose else (lambda *a, **k: None)
    say('Training size:', len(train_dataset), ' - Validation size:', len(val_dataset))

    if optimizer is None:
        if device.type == "cuda":
            from ..optim import FusedAdam
            optimizer = FusedAdam(model.parameters(), lr=lr, weight_decay=weight_decay)
        else:
            optimizer = optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)

    train_graph = train_dataset.get_graph(device)
    extra = [] if train_graph is None else [train_graph]
    held = pairs = None
    if resident is not False and (resident or not getattr(train_dataset, "resident_opt_in", False)):
        if ranking:
            pairs = train_dataset.resident_pairs(device) if device.type == "cuda" else None
        else:
            held = _resident_training_inputs(train_dataset, device, batch_size, per_batch_hook=resident is True)
    if resident and held is None and pairs is None:
        raise ValueError("resident training needs a CUDA device and a dataset with on-device batches")
    loader = None
    if held is None and pairs is None:
        loader = DataLoader(train_dataset, batch_size=batch_size, shuffle=shuffle, collate_fn=train_dataset.use_collate(), num_workers=num_workers)

    stopper = EarlyStopping(patience, max_patience, maximize=ranking)
    monitored_metrics = {'train_loss': [], 'val_loss': [], 'val_ndcg': []}
    best_ndcg = -1.0
    do_forward = train_dataset.__class__.do_forward
    n = len(train_dataset)

    for epoch in range(max_epochs):
        if ranking:
            train_dataset.w = schedule_w(epoch + 1)
        say(f'\nEpoch {epoch + 1}' + (f' (w = {train_dataset.w})' if ranking else ''))
        model.train()
        if pairs is not None:
            order = torch.randperm(n, device=device) if shuffle else torch.arange(n, device=device)
            seed = native.host_seed()    # torch's default (host) generator: no device sync
            running = torch.zeros((), dtype=torch.float64, device=device)
            for s in range(0, n, batch_size):
                batch = pairs.batch(order[s:s + batch_size], seed, s)   # slots numbered across the epoch
                optimizer.zero_grad()
                out_pos, out_neg = do_forward(model, batch, device, *extra)
                loss = train_dataset.calculate_loss(out_pos, out_neg)
                loss.backward()
                optimizer.step()
                running += loss.detach().double()
            train_sum_loss = float(running.item())   # the epoch's only host synchronisation
            pairs.check()                            # the sampler's flag and the out-of-range flag, already on the host's side
        elif held is not None:
            inputs, targets, on_batch = held
            order = torch.randperm(n, device=device) if shuffle else None
            running = torch.zeros((), dtype=torch.float64, device=device)
            for s in range(0, n, batch_size):
                pick = order[s:s + batch_size] if order is not None else slice(s, s + batch_size)
                batch = (*[t[pick] for t in inputs], targets[pick])
                if on_batch is not None:
                    batch = on_batch(*batch)
                optimizer.zero_grad()
                out, y = do_forward(model, batch, device, *extra)
                loss = train_dataset.calculate_loss(out, y)
                loss.backward()
                optimizer.step()
                running += loss.detach().double()
            train_sum_loss = float(running.item())   # the epoch's only host synchronisation
            if on_batch is not None:                 # batches built on the device: their sticky flags, already on the host's side
                native.check_pair_rows(device)
                native.check_oob(device)
        else:
            train_sum_loss = 0.0
            for batch in loader:
                optimizer.zero_grad()
                out, y = do_forward(model, batch, device, *extra)    # ranking: y is out_neg
                loss = train_dataset.calculate_loss(out, y.to(device))
                loss.backward()
                optimizer.step()
                train_sum_loss += loss.detach().item()
        train_loss = train_sum_loss / max(1, n)
        monitored_metrics['train_loss'].append(train_loss)
        say(f'Training loss: {train_loss:.4f}')

        val = eval_model(model, val_dataset, val_batch_size, ranking=ranking, device=device, resident=resident, cutoffs=(ndcg_cutoff,))
        val_ndcg, val_adj = val[f"ndcg@{ndcg_cutoff}"], val[f"adj_ndcg@{ndcg_cutoff}"]
        val_loss = None if ranking else val["mse"]
        if not ranking:
            monitored_metrics['val_loss'].append(val_loss)
        monitored_metrics['val_ndcg'].append(val_ndcg)
        val_dataset.samples['prediction'] = val["predictions"]   # as train.py:137 leaves it
        say((f'Validation loss: {val_loss:.4f} - ' if not ranking else '') +
            f'Validation NDCG@{ndcg_cutoff}: {val_ndcg:.4f}, adj-NDCG@{ndcg_cutoff}: {val_adj:.4f}')
        best_ndcg = max(best_ndcg, val_ndcg) if not np.isnan(val_ndcg) else best_ndcg
        if wandb is not None:
            logs = {'train_loss': train_loss, f'val_ndcg@{ndcg_cutoff}': val_ndcg, f'val_adj_ndcg@{ndcg_cutoff}': val_adj, 'epoch': epoch + 1}
            if ranking:
                logs['neg_sampling_w'] = train_dataset.w
            else:
                logs['val_loss'] = val_loss
            wandb.log(logs)

        if early_stop:
            verdict = stopper.update(val_ndcg if ranking else val_loss, epoch)
            if verdict == "best":
                model.save_model(checkpoint_model_path)
            elif verdict == "stop" or epoch == max_epochs - 1:
                say(f'{"Early stopping" if verdict == "stop" else "Last epoch"} at epoch {epoch + 1}: restoring the checkpoint of epoch '
                    f'{stopper.best_epoch + 1} (val {"ndcg" if ranking else "loss"} {stopper.best:.4f}).')
                state, _ = load_model(checkpoint_model_path, map_location=device)
                model.load_state_dict(state)
                model.eval()
                if verdict == "stop":
                    break
            say(f'Patience remaining: {patience - stopper.strikes}')

    if wandb is not None:
        logs = {'best_ndcg@10': best_ndcg}
        if stopper.best is not None and not ranking:
            logs['best_val_loss'] = stopper.best
        wandb.log(logs)
    if final_model_path is not None:
        model.save_model(final_model_path)
    return monitored_metrics
