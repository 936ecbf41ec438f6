"""torch.autograd wrappers that run a TRAINING step's forward and backward on the HIP kernels.

Only the differentiable building blocks of the scoring path are wrapped — the embedding gather and the Linear(+ReLU)
layers; loss, dropout masks and the optimizer stay torch ops (the reference's train loop, train.py:95-110, drives them).
  GatherConcatFn : forward ncf_gather_concat;  backward ncf_scatter_add_rows into dense table gradients
  LinearFn       : forward ncf_linear_forward (ReLU fused in the epilogue);
                   backward dX = dY . W (row-streaming GEMM with W^T), dW = dY^T . X (ncf_gemm_tn, ordered split over
                   the batch), db = ncf_colsum, ReLU mask = ncf_relu_backward_out
  SpmmFn         : LightGCN propagation y = A z (ncf_spmm_csr on the CSR by destination); backward dz = A^T dy = the SAME
                   kernel on the CSR by source (gnn_ncf.py:74-94 through autograd in the reference); optional per-edge
                   message dropout regenerated from a hash in both directions (ncf_spmm_csr_dropout)
  GatherPairOrderedFn : GatherConcatFn on one shared table with an ORDERED backward (stable sort of the ids + the segmented SpMM
                   instead of float atomics): the LightGAT step's readout, so a seeded run repeats itself bit for bit (table
                   widths that are a multiple of 4; others keep the atomics)
  GatSpmmFn      : LightGAT aggregation over the edges a step keeps: ncf_gat_edge_softmax + the SpmmFn kernels; backward dz as
                   SpmmFn, ds through ncf_gat_edge_grad (per-edge dot product, softmax backward per destination) and
                   ncf_gat_source_reduce (ordered sum per source over the transposed CSR)
  AttnFn         : grouped item-item attention (ncf_attn_forward_grouped) with its backward (ncf_attn_backward_grouped)
  DotSoftmaxLossFn : full-catalogue softmax cross-entropy of a dot-product readout without the B x N logits: forward ncf_dot_lse
                   + ncf_gather_dot for the target logits; backward ncf_dot_softmax_grad in its two roles, the user rows summed
                   into the table's gradient in a fixed order
"""
import torch

from . import native


class GatherConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tabA, idxA, tabB, idxB):
        ctx.save_for_backward(idxA, idxB)
        ctx.shapes = (tuple(tabA.shape), tuple(tabB.shape))
        return native.gather_concat(tabA.contiguous(), idxA, tabB.contiguous(), idxB)

    @staticmethod
    def backward(ctx, dX):
        idxA, idxB = ctx.saved_tensors
        (ra, ea), (rb, eb) = ctx.shapes
        dX = dX.contiguous()
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = torch.zeros((ra, ea), dtype=torch.float32, device=dX.device)
            native.scatter_add_rows(dX[:, :ea], idxA, dA)
        if ctx.needs_input_grad[2]:
            dB = torch.zeros((rb, eb), dtype=torch.float32, device=dX.device)
            native.scatter_add_rows(dX[:, ea:], idxB, dB)
        return dA, None, dB, None


class GatherColumnsFn(torch.autograd.Function):
    """x[p, :] = W[:, idx[p]] + b for the nn.Linear-layout embedding parameter W [E, U] (basic_ncf.py:25-33): what
    ``Linear(onehot(idx))`` computes.

    When W is stored id-major (util.row_major_embedding_: the transpose view of a contiguous [U, E] buffer — what
    BasicNCF / MF construct) this is a ROW gather, and the backward scatters 4·E-byte gradient rows (full-rate atomics)
    into a zeroed [U, E] buffer whose transpose VIEW is returned: the gradient has the parameter's own strides, so Adam
    runs elementwise over the raw buffers.  For a plain contiguous [E, U] weight the column kernels are used.  torch's
    ``W.t()[idx]`` backward goes through a sort and two table-sized copies either way.

    Row gradients: an id-major weight that carries a list attribute ``_ncf_row_grads`` (optim.RowSparseAdam marks its
    parameters so) gets NO dense gradient: backward appends ``(idx, dX)`` to that list and returns None for the weight — no
    table-sized zero fill, no scatter; the optimiser consumes the rows (native.adam_rows_)."""

    @staticmethod
    def forward(ctx, weight, bias, idx):
        ctx.save_for_backward(idx)
        ctx.wshape = tuple(weight.shape)
        ctx.has_bias = bias is not None
        ctx.row_major = weight.dim() == 2 and weight.t().is_contiguous() and not weight.is_contiguous()
        ctx.row_grads = getattr(weight, "_ncf_row_grads", None) if ctx.row_major else None
        if ctx.row_major:
            x = native.gather_concat(weight.t(), idx)
            return x if bias is None else x.add_(bias)
        return native.gather_cols(weight.contiguous(), None if bias is None else bias.contiguous(), idx)

    @staticmethod
    def backward(ctx, dX):
        (idx,) = ctx.saved_tensors
        dX = dX.contiguous()
        dW = db = None
        if ctx.needs_input_grad[0]:
            E, U = ctx.wshape
            if ctx.row_grads is not None:
                ctx.row_grads.append((idx, dX))
            elif ctx.row_major:
                dT = torch.zeros((U, E), dtype=torch.float32, device=dX.device)
                native.scatter_add_rows(dX, idx, dT)
                dW = dT.t()
            else:
                dW = torch.zeros((E, U), dtype=torch.float32, device=dX.device)
                native.scatter_add_cols(dX, idx, dW)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = native.colsum(dX)
        return dW, db, None


class GatherColumnsConcatFn(torch.autograd.Function):
    """cat(W_a[:, idx_a] + b_a, W_b[:, idx_b] + b_b) for two id-major embedding parameters in ONE gather into the (B, Ea+Eb)
    activation (``basic_ncf.py:37-40``: both embedding Linears, then the concat).  Against two GatherColumnsFn + torch.cat
    it saves the concat copy forward and, backward, the two column-slice copies and one of the two bias reductions: the
    gradient rows are scattered straight from the column halves of dX (the scatter kernel takes a row stride).  Both
    weights must be id-major (util.row_major_embedding_); the caller falls back to GatherColumnsFn + cat otherwise.  A weight
    marked with ``_ncf_row_grads`` (see GatherColumnsFn) receives ``(idx, its column half of dX)`` — a view, not a copy."""

    @staticmethod
    def forward(ctx, wa, ba, idx_a, wb, bb, idx_b):
        ctx.save_for_backward(idx_a, idx_b)
        ctx.row_grads = (getattr(wa, "_ncf_row_grads", None), getattr(wb, "_ncf_row_grads", None))
        ctx.shapes = (tuple(wa.shape), tuple(wb.shape))
        ctx.has_bias = (ba is not None, bb is not None)
        x = native.gather_concat(wa.t(), idx_a, wb.t(), idx_b)
        if ba is not None or bb is not None:
            ea, eb = wa.shape[0], wb.shape[0]
            bias = torch.cat((ba if ba is not None else x.new_zeros(ea), bb if bb is not None else x.new_zeros(eb)))
            x.add_(bias)
        return x

    @staticmethod
    def backward(ctx, dX):
        idx_a, idx_b = ctx.saved_tensors
        (ea, ua), (eb, ub) = ctx.shapes
        dX = dX.contiguous()
        d_wa = d_wb = d_ba = d_bb = None
        rows_a, rows_b = ctx.row_grads
        if ctx.needs_input_grad[0]:
            if rows_a is not None:
                rows_a.append((idx_a, dX[:, :ea]))
            else:
                ta = torch.zeros((ua, ea), dtype=torch.float32, device=dX.device)
                native.scatter_add_rows(dX[:, :ea], idx_a, ta)
                d_wa = ta.t()
        if ctx.needs_input_grad[3]:
            if rows_b is not None:
                rows_b.append((idx_b, dX[:, ea:]))
            else:
                tb = torch.zeros((ub, eb), dtype=torch.float32, device=dX.device)
                native.scatter_add_rows(dX[:, ea:], idx_b, tb)
                d_wb = tb.t()
        if (ctx.has_bias[0] and ctx.needs_input_grad[1]) or (ctx.has_bias[1] and ctx.needs_input_grad[4]):
            db = native.colsum(dX)
            d_ba = db[:ea] if ctx.has_bias[0] and ctx.needs_input_grad[1] else None
            d_bb = db[ea:] if ctx.has_bias[1] and ctx.needs_input_grad[4] else None
        return d_wa, d_ba, None, d_wb, d_bb, None


class SpmmFn(torch.autograd.Function):
    """y (N, D) = sum over the edges into each destination of coef_e * [dropout mask / (1 - p)] * z[src_e]  —  one LightGCN
    aggregation (gnn_ncf.py:52-70, 74-94).  ``prep`` is the PreparedGraph (CSR by destination + its transpose, built once per
    graph); ``coef`` the per-edge coefficients in CSR order (a training step recomputes them when it masks the batch's target
    edges); ``dropout`` = (p, seed) or None.  The coefficients are data, not parameters: no gradient flows to them."""

    @staticmethod
    def forward(ctx, z, prep, coef, dropout):
        ctx.prep, ctx.dropout = prep, dropout
        ctx.save_for_backward(coef)
        drop = None if dropout is None or dropout[0] <= 0 else (dropout[0], dropout[1], None)
        return prep.csr.spmm(z.contiguous(), coef=coef, dropout=drop)

    @staticmethod
    def backward(ctx, dY):
        (coef,) = ctx.saved_tensors
        prep = ctx.prep
        csr_t, eid = prep.transposed()
        drop = None if ctx.dropout is None or ctx.dropout[0] <= 0 else (ctx.dropout[0], ctx.dropout[1], eid)
        dZ = csr_t.spmm(dY.contiguous(), coef=coef[eid.long()], dropout=drop)   # same mask: entry e of A^T carries edge id eid[e]
        return dZ, None, None, None


def ordered_scatter_rows(src: torch.Tensor, idx: torch.Tensor, rows: int) -> torch.Tensor:
    """(rows, E) fp32: row r = the sum of the rows p of ``src`` (P, E) with idx[p] == r, in ascending p — GatherPairOrderedFn's
    fixed-order sum (a stable sort of the ids is the CSR the segmented SpMM reads), so equal inputs give equal bits.  Ids outside
    [0, rows) add nothing.  A width that is no multiple of 4 keeps ncf_scatter_add_rows (float atomics: not repeatable)."""
    e = src.shape[1]
    if e % 4:
        d = torch.zeros((rows, e), dtype=torch.float32, device=src.device)
        native.scatter_add_rows(src, idx, d)
        return d
    idx = torch.where((idx >= 0) & (idx < rows), idx, torch.full_like(idx, rows))           # bad ids: a spare row that is dropped
    rowptr = torch.zeros(rows + 2, dtype=torch.int64, device=src.device)
    rowptr[1:] = torch.cumsum(torch.bincount(idx, minlength=rows + 1), 0)
    order = torch.argsort(idx, stable=True).to(torch.int32)
    d = torch.empty((rows + 1, e), dtype=torch.float32, device=src.device)
    for c0 in range(0, e, 256):
        c1 = min(c0 + 256, e)
        native.spmm_csr(rowptr, None, order, None, src[:, c0:c1], rows + 1, y=d[:, c0:c1])
    return d[:rows]


class GatherPairOrderedFn(torch.autograd.Function):
    """cat(table[idxA], table[idxB]) — GatherConcatFn with both halves read from ONE table — whose backward adds the 2 B gradient
    rows of each table row in a fixed order: the ids are sorted (stable), and the sorted positions are the entries of a CSR by
    table row that the segmented SpMM sums without atomics (ncf_scatter_add_rows adds with float atomics, so its last bits depend
    on arrival order).  Ids outside the table get no gradient (the forward gather reports them).  The SpMM takes rows of at most 256
    floats, so wider tables (concat readouts) go through it in column blocks of 256.  A width that is no multiple of 4 cannot
    use the SpMM's 16-byte lanes and keeps the scatter kernel: such a step is NOT repeatable to the last bit."""

    @staticmethod
    def forward(ctx, table, idxA, idxB):
        ctx.save_for_backward(idxA, idxB)
        ctx.shape = tuple(table.shape)
        t = table.contiguous()
        return native.gather_concat(t, idxA, t, idxB)

    @staticmethod
    def backward(ctx, dX):
        idxA, idxB = ctx.saved_tensors
        rows, e = ctx.shape
        dX = dX.contiguous()
        if e % 4:
            d = torch.zeros((rows, e), dtype=torch.float32, device=dX.device)
            native.scatter_add_rows(dX[:, :e], idxA, d)
            native.scatter_add_rows(dX[:, e:], idxB, d)
            return d, None, None
        src = torch.cat((dX[:, :e], dX[:, e:]), dim=0)                # row p < B: the idxA half of pair p; row B + p: its idxB half
        return ordered_scatter_rows(src, torch.cat((idxA, idxB)), rows), None, None


class DotSoftmaxLossFn(torch.autograd.Function):
    """loss (B,) fp32: ``logsumexp_j(scale * <U[users[b]], Q[j]>) - scale * <U[users[b]], Q[targets[b]]>`` over EVERY row j of the
    item table Q (N, D) — softmax cross-entropy of the positive over the whole catalogue — for a user table U (rows, D) and
    ``users`` (B,) int64 rows of it (None: row b itself, B = rows).  Nothing of size B x N is built in either direction
    (csrc/dot_softmax.hip); the logits' scores are native.gather_dot's bits.

    Backward: dQ is dense (every item is in every denominator).  The B gradient rows of the users are summed into dU in a fixed
    order (ordered_scatter_rows), so a step repeats bit for bit; with ``users`` None they ARE dU — MF.softmax_loss passes the rows
    GatherColumnsFn gathered, whose backward hands (ids, rows) to optim.RowSparseAdam."""

    @staticmethod
    def forward(ctx, user_table, item_table, users, targets, scale):
        U, Q = user_table.contiguous(), item_table.contiguous()
        scale = native._finite("DotSoftmaxLossFn", scale, "scale")
        targets = targets.contiguous()
        lse = native.dot_lse(U, users, Q, None, scale)
        zt = native.gather_dot(U, users, Q, targets, B=targets.numel()).view(-1) * scale
        ctx.save_for_backward(U, Q, users, targets, lse)
        ctx.scale = scale
        return lse - zt

    @staticmethod
    def backward(ctx, g):
        U, Q, users, targets, lse = ctx.saved_tensors
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        dA, dQ = native.dot_softmax_grad(U, users, Q, None, targets, lse, g.contiguous().float(), ctx.scale, need=need)
        dU = None
        if dA is not None:
            dU = dA if users is None else ordered_scatter_rows(dA, users, U.shape[0])
        return dU, dQ, None, None, None


class GatSpmmFn(torch.autograd.Function):
    """y (N, D) = sum over the KEPT edges into each destination of attr_e * alpha_e * [dropout mask / (1 - p)] * z[src_e], alpha the
    per-destination softmax of the source scores s[src_e] over the kept edges  —  one LightGAT aggregation (gnn_ncf.py:151-177).
    ``z`` (N, D) is the hoisted per-node Linear, ``s`` (N, 1) the source half of AttNet applied per node; ``prep`` the PreparedGraph;
    ``keep`` the per-entry 1 / 0 indicator of the step's edge set (native.edge_keep with attr = None) or None; ``dropout`` = (p, seed)
    or None.  ``att_zero_params``: AttNet's weight(s) and bias(es), taken only to hand them a gradient that is exactly zero — the
    destination half of the score and the bias are constant inside a softmax group and cancel (the source half of the weight gets
    its real gradient through ``s``), so an optimizer sees a gradient for every parameter, as on the torch path."""

    @staticmethod
    def forward(ctx, z, s, prep, keep, dropout, *att_zero_params):
        z, sv = z.contiguous(), s.contiguous().view(-1)
        seg = prep.softmax_segments()
        seg_first = None if seg is None else seg[2]
        alpha, coef = native.gat_edge_softmax(prep.segptr, prep.row_of, seg_first, prep.N, prep.col, prep.attr, keep, sv,
                                              workspace=prep.gat_workspace())
        ctx.prep, ctx.dropout, ctx.seg_first, ctx.s_shape = prep, dropout, seg_first, tuple(s.shape)
        ctx.save_for_backward(z, alpha, coef, *att_zero_params)
        drop = None if dropout is None or dropout[0] <= 0 else (dropout[0], dropout[1], None)
        return prep.csr.spmm(z, coef=coef, dropout=drop)

    @staticmethod
    def backward(ctx, dY):
        z, alpha, coef, *zero_params = ctx.saved_tensors
        prep = ctx.prep
        dY = dY.contiguous()
        csr_t, eid = prep.transposed()
        on = ctx.dropout is not None and ctx.dropout[0] > 0
        dZ = ds = None
        if ctx.needs_input_grad[0]:
            dZ = csr_t.spmm(dY, coef=coef[eid.long()], dropout=(ctx.dropout[0], ctx.dropout[1], eid) if on else None)
        if ctx.needs_input_grad[1]:
            p, seed = ctx.dropout if on else (0.0, 0)
            dlogit = native.gat_edge_grad(prep.segptr, prep.row_of, ctx.seg_first, prep.N, prep.col, prep.attr, alpha, dY, z, p, seed,
                                          workspace=prep.gat_workspace())
            ds = native.gat_source_reduce(csr_t, eid, dlogit).view(ctx.s_shape)
        zeros = tuple(torch.zeros_like(q) if ctx.needs_input_grad[5 + k] else None for k, q in enumerate(zero_params))
        return (dZ, ds, None, None, None) + zeros


class AttnFn(torch.autograd.Function):
    """user_emb (B, UE) = bias + sum_e softmax_e(score(b, e)) * val_e * proj[col_e, :]  —  attention_ncf.py:176-216 for one CSR row
    of rated entries per pair, forward (ncf_attn_forward / _dropout) and backward (ncf_attn_backward) on the HIP kernels.
    ``b1`` (AttentionNet's output bias) is taken only to hand it its gradient, which is exactly zero: a shift of every score
    cancels in the softmax.  ``dropout`` = (p, seed) or None: AttentionNet's hidden dropout, regenerated in both kernels.
    ``msg_dropout`` = (p, seed) or None: the message dropout over the logits (ncf_attn_forward_train / _backward_train).  With it the
    value of ``b1`` does reach the kernel: the reference's ``attOut == 0`` test is made on the score with its bias, so an entry whose
    hidden units are all inactive is kept with score b1, not dropped.  That is one 4-byte host read per step, on this path only:
    a blocking read (the step waits for the queued work before it), and one that cannot be made inside a stream capture — a step with
    message dropout on the device cannot be captured into a HIP graph.  11-argument callers leave ``msg_dropout`` at None."""

    @staticmethod
    def forward(ctx, pc, pr, w1, b1, proj, bias, rowptr, col, val, mode, dropout, msg_dropout=None):
        pc, pr, proj = pc.contiguous(), pr.contiguous(), proj.contiguous()
        w1c = None if w1 is None else w1.contiguous()
        msg_on = msg_dropout is not None and msg_dropout[0] > 0
        b1v = float(b1.detach().reshape(-1)[0].item()) if msg_on and b1 is not None else 0.0
        out, wts = native.attn_forward(mode, pc, pr, w1c, b1v, rowptr, col, val, proj, out_bias=bias, dropout=dropout,
                                       **({"msg_dropout": msg_dropout} if msg_on else {}))
        ctx.mode, ctx.dropout, ctx.msg_dropout = mode, dropout, (msg_dropout if msg_on else None)
        ctx.has = (w1 is not None, b1 is not None, bias is not None)
        ctx.save_for_backward(pc, pr, w1c, proj, rowptr, col, val, wts)
        ctx.mark_non_differentiable(wts)
        return out, wts

    @staticmethod
    def backward(ctx, dout, _dwts):
        pc, pr, w1c, proj, rowptr, col, val, wts = ctx.saved_tensors
        d_pc, d_pr, d_w1, d_proj = native.attn_backward(ctx.mode, pc, pr, w1c, rowptr, col, val, proj, wts, dout, dropout=ctx.dropout,
                                                        **({"msg_dropout": ctx.msg_dropout} if ctx.msg_dropout else {}))
        has_w1, has_b1, has_bias = ctx.has
        d_b1 = torch.zeros(1, dtype=torch.float32, device=dout.device) if has_b1 else None
        d_bias = native.colsum(dout.contiguous()) if has_bias else None
        # one gradient slot per forward argument; autograd drops a trailing None when the caller passed 11
        return d_pc, d_pr, (d_w1 if has_w1 else None), d_b1, d_proj, d_bias, None, None, None, None, None, None


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        x = x.contiguous()
        w = weight.contiguous()
        y = native.linear_act(x, w, None if bias is None else bias.contiguous(), relu)
        ctx.relu = bool(relu)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, w, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dY):
        x, w, y = ctx.saved_tensors
        dY = dY.contiguous()
        if ctx.relu:
            dY = native.relu_backward(dY, y)   # one pass into a new buffer: the incoming gradient is not ours to modify
        dX = dW = db = None
        if ctx.needs_input_grad[0]:
            if w.shape[0] == 1:
                dX = dY * w          # 1-wide output layer: dX is the outer product (one exact product per element, no GEMM)
            else:
                dX = native.linear_act(dY, w.t().contiguous(), None, False)   # dX = dY . W
        if ctx.needs_input_grad[1]:
            dW = native.gemm_tn(dY, x)                                   # dW = dY^T . X
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = native.colsum(dY)
        return dX, dW, db, None


class LinearReluDropoutFn(torch.autograd.Function):
    """dropout(relu(x W^T + b), p) — the reference's hidden-layer block in training mode (util.py:12-17) — as ONE autograd
    node.  Forward: the HIP Linear with the ReLU in its epilogue, then torch's dropout (its Philox stream, so a seeded run
    draws the masks it would draw with plain torch ops).  Only the OUTPUT z is kept: z > 0 exactly where the ReLU was
    active and the element survived, so the backward of both is ``dz * 1/(1-p)`` masked by ``z > 0`` — one pass of
    ncf_relu_backward_out instead of torch's masked-scale kernel plus the ReLU mask, and neither the pre-dropout
    activation nor the mask is stored."""

    @staticmethod
    def forward(ctx, x, weight, bias, p):
        x = x.contiguous()
        w = weight.contiguous()
        z = torch.nn.functional.dropout(native.linear_act(x, w, None if bias is None else bias.contiguous(), True), p, True)
        ctx.scale = 1.0 / (1.0 - p)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, w, z)
        return z

    @staticmethod
    def backward(ctx, dZ):
        x, w, z = ctx.saved_tensors
        dY = native.relu_backward(dZ.contiguous(), z, ctx.scale)
        dX = dW = db = None
        if ctx.needs_input_grad[0]:
            dX = native.linear_act(dY, w.t().contiguous(), None, False)
        if ctx.needs_input_grad[1]:
            dW = native.gemm_tn(dY, x)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = native.colsum(dY)
        return dX, dW, db, None


def mlp_train(seq: torch.nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """A build_MLP_layers Sequential (Linear, [ReLU, Dropout?, Linear]*) applied with the HIP autograd blocks: every
    Linear that is followed by a ReLU fuses it, and a training-mode Dropout behind that joins the same node
    (LinearReluDropoutFn); any other module runs as the torch op it is."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, torch.nn.Linear):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
            drop = mods[i + 2] if fuse and i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.Dropout) else None
            if drop is not None and drop.training and 0.0 < drop.p < 1.0 and not drop.inplace:
                x = LinearReluDropoutFn.apply(x, m.weight, m.bias, float(drop.p))
                i += 3
                continue
            x = LinearFn.apply(x, m.weight, m.bias, fuse)
            i += 2 if fuse else 1
        else:
            x = m(x)
            i += 1
    return x
