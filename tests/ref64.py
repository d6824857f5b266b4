"""Float64 numpy reference of the tick operations and the evaluation
metrics, written from the handler semantics and independent of
``TorchBackend``: local SGD updates and in-order deliveries for logreg
(plain, limited-merge, partitioned) and the MLP (plain, limited-merge), and
the classification metrics of ``gossipy_amd.engine.metrics``.

The tests measure the fp32 oracle and the HIP kernels against it, so it is
kept plain: one sample batch at a time, dense matrix products, no in-place
tricks. Not a test module (no ``test_`` prefix); the test files next to it
import it by name.

``broken=(T, kind)`` reproduces a per-sample stage that only covers the
first ``T`` rows of a batch: the ``dz`` rows from ``T`` on are left as zeros
(``kind="zero"``) or as the raw forward scores (``kind="scores"``). It is
used to show that a case's inputs can see such a defect.
"""

import numpy as np

from gossipy_amd.core import CreateModelMode

MERGE_UPDATE = CreateModelMode.MERGE_UPDATE
UPDATE = CreateModelMode.UPDATE
UPDATE_MERGE = CreateModelMode.UPDATE_MERGE
PASS = CreateModelMode.PASS


# -- one minibatch step per family -------------------------------------------

def _softmax(a):
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _onehot(y, k):
    out = np.zeros((len(y), k))
    out[np.arange(len(y)), y] = 1.0
    return out


def _break(dz, raw, broken):
    if broken is not None:
        T, kind = broken
        dz[T:] = 0.0 if kind == "zero" else raw[T:]
    return dz


def _logreg_grad(spec, row, xb, yb, broken):
    """Flat gradient of CE(softmax(sigmoid(xW' + b))) over one batch."""
    d, k = spec.d_in, spec.n_classes
    W, b = row[: k * d].reshape(k, d), row[k * d:]
    m = xb.shape[0]
    z = xb @ W.T + b
    a = 1.0 / (1.0 + np.exp(-z))
    dz = (_softmax(a) - _onehot(yb, k)) / m * a * (1.0 - a)
    dz = _break(dz, z, broken)
    return np.concatenate([(dz.T @ xb).reshape(-1), dz.sum(axis=0)])


def _logreg_step(spec, row, xb, yb, broken):
    d, k = spec.d_in, spec.n_classes
    g = _logreg_grad(spec, row, xb, yb, broken)
    if spec.weight_decay:  # weights only
        g[: k * d] += spec.weight_decay * row[: k * d]
    row -= spec.lr * g


def _mlp_grad(spec, row, xb, yb, broken):
    """Flat gradient of CE(softmax(head)) for the ReLU MLP, every layer's
    gradient taken at the pre-step weights."""
    offs = spec.layer_offsets()
    m = xb.shape[0]
    acts = [xb]
    h = xb
    for li, (w_off, b_off, fin, fout) in enumerate(offs):
        h = h @ row[w_off:b_off].reshape(fout, fin).T + row[b_off:b_off + fout]
        if li < len(offs) - 1:
            h = np.maximum(h, 0.0)
        acts.append(h)
    k = offs[-1][3]
    dh = (_softmax(h) - _onehot(yb, k)) / m
    dh = _break(dh, h, broken)
    g = np.zeros_like(row)
    for li in reversed(range(len(offs))):
        w_off, b_off, fin, fout = offs[li]
        g[w_off:b_off] = (dh.T @ acts[li]).reshape(-1)
        g[b_off:b_off + fout] = dh.sum(axis=0)
        if li > 0:
            dh = (dh @ row[w_off:b_off].reshape(fout, fin)) * (acts[li] > 0)
    return g


def _mlp_step(spec, row, xb, yb, broken):
    g = _mlp_grad(spec, row, xb, yb, broken)
    if spec.weight_decay:  # weights only in the plain step
        for (w_off, b_off, _, _) in spec.layer_offsets():
            g[w_off:b_off] += spec.weight_decay * row[w_off:b_off]
    row -= spec.lr * g


def _train(spec, row, age, x, y, broken=None):
    """All local epochs of one node on its shard ``x [c, d]``, ``y [c]``.
    ``row`` is updated in place; returns the new age (a scalar, or the
    partition age vector for a partitioned spec)."""
    c = x.shape[0]
    if c == 0:
        return age
    part = getattr(spec, "n_parts", 0) > 0
    grad = _logreg_grad if spec.family == "logreg" else _mlp_grad
    step = _logreg_step if spec.family == "logreg" else _mlp_step
    bs = c if spec.batch_size == 0 else spec.batch_size
    for _ in range(max(1, spec.local_epochs)):
        for s in range(0, c, bs):
            xb, yb = x[s:s + bs], y[s:s + bs]
            if part:
                # the whole age vector is bumped before the step and each
                # parameter's gradient is divided by its partition's age;
                # the decay then covers the whole row
                age = age + 1
                g = grad(spec, row, xb, yb, broken)
                g /= age[spec.arena_part()].astype(np.float64)
                if spec.weight_decay:
                    g += spec.weight_decay * row
                row -= spec.lr * g
            else:
                step(spec, row, xb, yb, broken)
                age = age + 1
    return age


# -- merges --------------------------------------------------------------------

def _merge(spec, row, age, srow, sage):
    """Mean merge, or the limited merge when the spec has a threshold: keep
    when a > b + L, adopt when b > a + L, else a/(a+b), b/(a+b) weights
    ((1/2, 1/2) when a + b == 0). The age becomes max(a, b)."""
    L = getattr(spec, "age_diff_threshold", None)
    a, b = int(age), int(sage)
    if L is None:
        row[:] = 0.5 * (row + srow)
    elif a > b + L:
        pass
    elif b > a + L:
        row[:] = srow
    elif a + b == 0:
        row[:] = 0.5 * row + 0.5 * srow
    else:
        row[:] = (a / (a + b)) * row + (b / (a + b)) * srow
    return max(a, b)


def _merge_part(spec, row, agev, srow, sagev, pid):
    """Age-weighted merge of partition ``pid`` alone (weights (0, 0) count
    as (1, 1)); only that partition's age moves."""
    ptr, perm = spec.part_ptr(), spec.part_perm()
    idx = perm[ptr[pid]:ptr[pid + 1]]
    w1, w2 = int(agev[pid]), int(sagev[pid])
    if w1 == 0 and w2 == 0:
        w1 = w2 = 1
    row[idx] = (w1 / (w1 + w2)) * row[idx] + (w2 / (w1 + w2)) * srow[idx]
    agev = agev.copy()
    agev[pid] = max(int(agev[pid]), int(sagev[pid]))
    return agev


# -- the two operations ----------------------------------------------------------

class RefState:
    """float64 / int64 copies of a NodeStateArena, a SlotPool and a
    DataArena (any of the torch CPU objects the engine uses)."""

    def __init__(self, state, data, pool=None):
        self.params = state.params.double().numpy().copy()
        self.ages = state.ages.long().numpy().copy()
        self.x = data.x.double().numpy()
        self.y = data.y.long().numpy()
        self.counts = data.counts.long().numpy()
        if pool is not None:
            self.slots = pool.slots.double().numpy().copy()
            self.slot_ages = pool.slot_ages.long().numpy().copy()

    def shard(self, node):
        c = int(self.counts[node])
        return self.x[node, :c], self.y[node, :c]


def update(spec, rs, nodes, broken=None):
    for node in [int(v) for v in nodes]:
        x, y = rs.shard(node)
        rs.ages[node] = _train(spec, rs.params[node], rs.ages[node], x, y,
                               broken)


def deliver(spec, rs, recv_nodes, recv_ptr, del_slots, reply_slots,
            del_pids=None, broken=None):
    """Per receiver row, its deliveries in order; a reply slot receives the
    row as it stands right after its own delivery. Delivered slots are only
    read."""
    part = getattr(spec, "n_parts", 0) > 0
    pt = getattr(spec, "pass_through", False)
    ptr = [int(v) for v in recv_ptr]
    for i, node in enumerate(int(v) for v in recv_nodes):
        x, y = rs.shard(node)
        row = rs.params[node]
        age = rs.ages[node].copy()
        for j in range(ptr[i], ptr[i + 1]):
            slot = int(del_slots[j])
            srow = rs.slots[slot].copy()
            sage = rs.slot_ages[slot].copy()
            mode = spec.mode
            if part:
                pid = int(del_pids[j])
                if mode == MERGE_UPDATE:
                    age = _merge_part(spec, row, age, srow, sage, pid)
                    age = _train(spec, row, age, x, y, broken)
                elif mode in (UPDATE, UPDATE_MERGE):
                    if mode == UPDATE_MERGE:
                        age = _train(spec, row, age, x, y, broken)
                    sage = _train(spec, srow, sage, x, y, broken)
                    age = _merge_part(spec, row, age, srow, sage, pid)
                else:
                    raise ValueError("PASS is not allowed when partitioned")
            else:
                if pt and del_pids is not None and int(del_pids[j]) == 1:
                    mode = PASS
                if mode == MERGE_UPDATE:
                    age = _merge(spec, row, age, srow, sage)
                    age = _train(spec, row, age, x, y, broken)
                elif mode == UPDATE:
                    row[:] = srow
                    age = _train(spec, row, sage, x, y, broken)
                elif mode == UPDATE_MERGE:
                    age = _train(spec, row, age, x, y, broken)
                    sage = _train(spec, srow, sage, x, y, broken)
                    age = _merge(spec, row, age, srow, sage)
                else:  # PASS
                    row[:] = srow
                    age = sage
            r = int(reply_slots[j])
            if r >= 0:
                rs.slots[r] = row
                rs.slot_ages[r] = age
        rs.ages[node] = age


# -- metrics ---------------------------------------------------------------------

def rank_auc(score, pos):
    """Mann-Whitney AUC with average ranks for ties; 0.5 when a class is
    missing. ``score [n]``, ``pos [n]`` boolean."""
    score = np.asarray(score, dtype=np.float64)
    pos = np.asarray(pos, dtype=bool)
    npos, nneg = int(pos.sum()), int((~pos).sum())
    if npos == 0 or nneg == 0:
        return 0.5
    vals, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])  # 0-based start
    avg_rank = first + (cnt + 1) / 2.0  # mean of first+1 .. first+cnt
    ranks = avg_rank[inv]
    return float((ranks[pos].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


def _macro(pred, true, k):
    conf = np.zeros((k, k))
    np.add.at(conf, (true, pred), 1.0)
    tp = np.diag(conf)
    pred_tot, true_tot = conf.sum(axis=0), conf.sum(axis=1)
    p = np.where(pred_tot > 0, tp / np.maximum(pred_tot, 1), 0.0)
    r = np.where(true_tot > 0, tp / np.maximum(true_tot, 1), 0.0)
    f = np.where(p + r > 0, 2 * p * r / np.maximum(p + r, 1e-300), 0.0)
    return {
        "accuracy": float((pred == true).mean()),
        "precision": float(p.mean()),
        "recall": float(r.mean()),
        "f1_score": float(f.mean()),
    }


def class_metrics(scores, y):
    """Metrics of one model from its class scores ``[n, k]`` and labels
    ``[n]``: accuracy, macro precision / recall / F1 (a class without
    predictions or without samples contributes 0), and for ``k == 2`` the
    AUC of the class-1 score. The first maximal score wins the argmax."""
    scores = np.asarray(scores, dtype=np.float64)
    y = np.asarray(y).astype(np.int64)
    k = scores.shape[1]
    out = _macro(scores.argmax(axis=1), y, k)
    if k == 2:
        out["auc"] = rank_auc(scores[:, 1], y == 1)
    return out


def margin_metrics(margin, y):
    """Metrics of a margin model: prediction +1 where ``margin >= 0``,
    labels in {-1, +1}, classes ordered (-1, +1)."""
    margin = np.asarray(margin, dtype=np.float64)
    yt = (np.asarray(y) > 0).astype(np.int64)
    out = _macro((margin >= 0).astype(np.int64), yt, 2)
    out["auc"] = rank_auc(margin, yt == 1)
    return out


def logreg_scores(row, X, d, k):
    """Raw affine class scores ``[n, k]`` of a logreg row (the sigmoid is
    monotonic, so argmax and ranks are those of the probabilities)."""
    row = np.asarray(row, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    return X @ row[: k * d].reshape(k, d).T + row[k * d:]
