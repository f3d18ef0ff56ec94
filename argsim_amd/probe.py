"""linear probes of latent rows: the downstream classification of the reference's src/eval_classification.py (a one-vs-rest L2
logistic regression per topic, scored by cross-validation) as ONE batched fit on the device (include/argsim_vae.h, avae_probe_fit).

    probe_costs(labels, train_idx, C, class_weight)  liblinear's weighting as signed per-row costs: pure numpy
    fit(vae, z, labels, ...)                         -> Probe (classes_, coef_, intercept_, stats, decision, predict)
    cross_validate(vae, z, labels, folds, groups)    every group x fold x class in one avae_probe_fit -> held-out predictions, scores
    l1_costs / fit_l1 / select_dims(vae, z, labels)  the L1 model of src/eval_clustering.py:46-58 (avae_probe_fit_l1) and the columns it keeps
"""
import ctypes as C

import numpy as np

DEFAULT_TOL = 1e-4          # scikit-learn's; DESIGN 4.3h records the smallest tol at which every test case still converges
DEFAULT_MAX_NEWTON = 50
DEFAULT_MAX_CG = 30
DEFAULT_MAX_INNER = 50      # the L1 fit: Hessian products per proximal Newton iteration
STATUS = {0: 'converged', 1: 'max_newton reached', 2: 'line search exhausted or a value that is not finite'}


def probe_costs(labels, train_idx=None, C=0.001, class_weight='balanced'):
    """liblinear's one-vs-rest weighting of LogisticRegression(C, penalty='l2', solver='liblinear', class_weight) on the rows
    train_idx of labels (N,), as the signed costs avae_probe_fit takes -> (classes, costs): classes the sorted labels present among
    the training rows (K of them), costs (P, N) float32.  With w_k = |T| / (K n_k) (balanced; else 1):
        K >= 3   P = K: problem k has +C w_k on the training rows of class k and -C on the other training rows
        K == 2   P = 1: +C w_1 on the rows of the larger class (classes[1]), -C w_0 on the others; a positive decision predicts it
        K == 1   P = 0: the constant prediction
    and 0 on every row outside train_idx: such a row is not in the problem."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] < 1:
        raise ValueError("labels must be (N,) with N >= 1, got %s" % (labels.shape,))
    if class_weight not in ('balanced', None):
        raise ValueError("class_weight must be 'balanced' or None, got %r" % (class_weight,))
    if isinstance(C, bool) or not np.isfinite(C) or not C > 0:
        raise ValueError("C must be a finite number > 0, got %r" % (C,))
    N = labels.shape[0]
    if train_idx is None:
        train_idx = np.arange(N)
    train_idx = np.asarray(train_idx)
    if train_idx.dtype == np.bool_:
        if train_idx.shape != (N,):
            raise ValueError("a boolean train mask must be (N,) = (%d,), got %s" % (N, train_idx.shape))
        train_idx = np.flatnonzero(train_idx)
    if train_idx.ndim != 1 or train_idx.shape[0] < 1 or not np.issubdtype(train_idx.dtype, np.integer):
        raise ValueError("train_idx must be a non-empty 1-d integer index or a boolean mask")
    if train_idx.min() < 0 or train_idx.max() >= N or np.unique(train_idx).shape[0] != train_idx.shape[0]:
        raise ValueError("train_idx must hold distinct row numbers in [0, %d)" % N)
    classes, inv, counts = np.unique(labels[train_idx], return_inverse=True, return_counts=True)
    K, T = classes.shape[0], train_idx.shape[0]
    wk = T / (K * counts.astype(np.float64)) if class_weight == 'balanced' else np.ones(K)
    P = K if K >= 3 else K - 1
    costs = np.zeros((P, N), np.float64)
    if K >= 3:
        for k in range(K):
            costs[k, train_idx] = np.where(inv == k, C * wk[k], -C)
    elif K == 2:
        costs[0, train_idx] = np.where(inv == 1, C * wk[1], -C * wk[0])
    return classes, costs.astype(np.float32)


def l1_costs(labels, train_idx=None, C=0.1, class_weight=None):
    """the signed costs of the reference's dimension selection, LogisticRegression(penalty='l1', C=0.1, solver='liblinear') of
    src/eval_clustering.py:46: the one-vs-rest layout of probe_costs (K >= 3: K problems, K = 2: one, K = 1: none) with that
    call's defaults, C = 0.1 and no class weights -> (classes, costs (P, N) float32) for avae_probe_fit_l1"""
    return probe_costs(labels, train_idx, C, class_weight)


def _check_fit_args(z, costs, tol, max_newton, max_cg, inner='max_cg'):
    """the argument rules of avae_probe_fit (and, with inner='max_inner', of avae_probe_fit_l1), checked before anything touches
    the device"""
    _check_rows('z', z)
    if not isinstance(costs, np.ndarray) or costs.dtype != np.float32 or costs.ndim != 2:
        raise ValueError("costs must be a (P, N) float32 numpy array")
    if costs.shape[0] < 1 or costs.shape[1] != z.shape[0]:
        raise ValueError("costs must be (P, N) with P >= 1 and N = %d rows of z, got %s" % (z.shape[0], costs.shape))
    for name, v in (('max_newton', max_newton), (inner, max_cg)):
        if isinstance(v, bool) or int(v) != v or not 1 <= v < (1 << 31):
            raise ValueError("%s must be an integer >= 1, got %r" % (name, v))
    if isinstance(tol, bool) or not (tol >= 0) or not np.isfinite(tol):
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    return float(tol), int(max_newton), int(max_cg)


def _check_rows(name, x):
    import torch
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError("%s must be a numpy array or a torch tensor, got %s" % (name, type(x).__name__))
    if x.dtype not in (np.float32, torch.float32):
        raise ValueError("%s must be float32, got %s" % (name, x.dtype))
    if len(x.shape) != 2 or x.shape[0] < 1:
        raise ValueError("%s must be (rows, dim) with at least one row, got %s" % (name, tuple(x.shape)))
    if x.shape[0] > (1 << 31) - 256:
        raise ValueError("at most 2^31 - 256 rows per call, got %d" % x.shape[0])
    dim = x.shape[1]
    if dim % 4 or not 4 <= dim <= 1024:
        raise ValueError("dim must be a multiple of 4 in [4, 1024], got %d" % (dim,))
    if isinstance(x, torch.Tensor) and x.is_contiguous() and x.data_ptr() % 16:
        raise ValueError("%s must be 16-byte aligned (a view that starts inside a row block is not)" % name)


def fit_raw(vae, z, costs, tol=DEFAULT_TOL, max_newton=DEFAULT_MAX_NEWTON, max_cg=DEFAULT_MAX_CG):
    """avae_probe_fit as it stands: z (N, dim) float32 numpy or torch, costs (P, N) float32 numpy -> (w (P, dim + 1), stats (P, 4)) numpy"""
    from . import lib as _lib
    tol, max_newton, max_cg = _check_fit_args(z, costs, tol, max_newton, max_cg)
    return _fit_call(vae, z, costs, vae._l.avae_probe_fit, _lib.AvaeProbeConfig(max_newton, max_cg, tol, 0))


def _fit_call(vae, z, costs, entry, pc):
    """one of the two fit entries (same arguments but for the config) on checked arguments"""
    import torch
    x = vae._dev_f32(z)
    s = torch.as_tensor(np.ascontiguousarray(costs)).to(vae.device)
    N, dim, P = x.shape[0], x.shape[1], costs.shape[0]
    w = torch.empty((P, dim + 1), dtype=torch.float32, device=vae.device)
    stats = torch.empty((P, 4), dtype=torch.float32, device=vae.device)
    vae._stream()
    vae._ck(entry(vae._h, C.c_void_p(x.data_ptr()), N, dim, C.c_void_p(s.data_ptr()), P, C.byref(pc),
                  C.c_void_p(w.data_ptr()), C.c_void_p(stats.data_ptr())))
    return w.cpu().numpy(), stats.cpu().numpy()


def fit_l1_raw(vae, z, costs, tol=DEFAULT_TOL, max_newton=DEFAULT_MAX_NEWTON, max_inner=DEFAULT_MAX_INNER):
    """avae_probe_fit_l1 as it stands: z (N, dim) float32 numpy or torch, costs (P, N) float32 numpy -> (w (P, dim + 1), stats (P, 4))
    numpy; a zero of w is an exact +0.0"""
    from . import lib as _lib
    tol, max_newton, max_inner = _check_fit_args(z, costs, tol, max_newton, max_inner, 'max_inner')
    return _fit_call(vae, z, costs, vae._l.avae_probe_fit_l1, _lib.AvaeProbeL1Config(max_newton, max_inner, tol, 0))


def decision_raw(vae, z, w):
    """avae_probe_decision: z (n, dim), w (P, dim + 1) -> (n, P) float32 numpy"""
    import torch
    _check_rows('z', z)
    if not isinstance(w, np.ndarray) or w.dtype != np.float32 or w.ndim != 2 or w.shape[0] < 1 or w.shape[1] != z.shape[1] + 1:
        raise ValueError("w must be a (P, dim + 1) float32 numpy array with P >= 1 and dim = %d" % z.shape[1])
    x = vae._dev_f32(z)
    dw = torch.as_tensor(np.ascontiguousarray(w)).to(vae.device)
    out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=vae.device)
    vae._stream()
    vae._ck(vae._l.avae_probe_decision(vae._h, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], C.c_void_p(dw.data_ptr()), w.shape[0],
                                       C.c_void_p(out.data_ptr())))
    return out.cpu().numpy()


def labels_from_decision(classes, dec):
    """the prediction rule of the one-vs-rest model: dec (n, P) -> labels (n,).  K >= 3: the first maximum (numpy's argmax); K = 2:
    classes[1] where the one decision is positive; K = 1: the constant"""
    K = len(classes)
    if K == 1:
        return np.repeat(classes[:1], dec.shape[0])
    if K == 2:
        return classes[(dec[:, 0] > 0).astype(np.int64)]
    return classes[np.argmax(dec, axis=1)]


class Probe:
    """a fitted one-vs-rest model: classes_ (K,), coef_ (P, dim), intercept_ (P,), stats (P, 4) = f, |grad f|, Newton iterations,
    status per problem (P = K, or 1 for K = 2, or 0 for K = 1); of an L1 fit: F, |v|_1, outer iterations, status"""

    def __init__(self, vae, classes, w, stats):
        self._vae, self.classes_, self._w, self.stats = vae, classes, w, stats
        self.coef_, self.intercept_ = w[:, :-1], w[:, -1]

    def decision(self, z):
        if self._w.shape[0] == 0:
            _check_rows('z', z)
            return np.zeros((z.shape[0], 0), np.float32)
        return decision_raw(self._vae, z, self._w)

    def predict(self, z):
        return labels_from_decision(self.classes_, self.decision(z))


def _check_labels(z, labels, name='labels'):
    _check_rows('z', z)
    labels = np.asarray(labels)
    if labels.shape != (z.shape[0],):
        raise ValueError("%s must be (N,) = (%d,), got %s" % (name, z.shape[0], labels.shape))
    return labels


def fit(vae, z, labels, C=0.001, class_weight='balanced', train=None, tol=DEFAULT_TOL, max_newton=DEFAULT_MAX_NEWTON, max_cg=DEFAULT_MAX_CG):
    labels = _check_labels(z, labels)
    classes, costs = probe_costs(labels, train, C, class_weight)
    dim = z.shape[1]
    if costs.shape[0] == 0:
        _check_fit_args(z, np.zeros((1, z.shape[0]), np.float32), tol, max_newton, max_cg)
        return Probe(vae, classes, np.zeros((0, dim + 1), np.float32), np.zeros((0, 4), np.float32))
    w, stats = fit_raw(vae, z, costs, tol, max_newton, max_cg)
    return Probe(vae, classes, w, stats)


def fit_l1(vae, z, labels, C=0.1, class_weight=None, train=None, tol=DEFAULT_TOL, max_newton=DEFAULT_MAX_NEWTON, max_inner=DEFAULT_MAX_INNER):
    """the one-vs-rest L1 model of the labels (l1_costs) fitted by avae_probe_fit_l1 -> Probe; its stats are F, |v|_1, the outer
    iterations and the status per problem"""
    labels = _check_labels(z, labels)
    classes, costs = l1_costs(labels, train, C, class_weight)
    dim = z.shape[1]
    if costs.shape[0] == 0:
        _check_fit_args(z, np.zeros((1, z.shape[0]), np.float32), tol, max_newton, max_inner, 'max_inner')
        return Probe(vae, classes, np.zeros((0, dim + 1), np.float32), np.zeros((0, 4), np.float32))
    w, stats = fit_l1_raw(vae, z, costs, tol, max_newton, max_inner)
    return Probe(vae, classes, w, stats)


def useful_dims(coef):
    """the rule of the reference's src/eval_clustering.py:57 on coef (P, dim): the sorted numbers of the columns with a nonzero
    coefficient in any class (int64, as useful_dimension.npy).  The device returns exact zeros, so no threshold is used."""
    coef = np.asarray(coef)
    if coef.ndim != 2:
        raise ValueError("coef must be (P, dim), got %s" % (coef.shape,))
    return np.flatnonzero((coef != 0).any(axis=0)).astype(np.int64)


def select_dims(vae, z, labels, C=0.1, class_weight=None, train=None, **solver):
    """the dimension selection of src/eval_clustering.py:46-58 -> (dims, probe): the L1 model of the labels and the columns of z it
    uses.  solver: tol, max_newton, max_inner."""
    probe = fit_l1(vae, z, labels, C, class_weight, train, **solver)
    return useful_dims(probe.coef_), probe


def cv_problems(labels, folds, groups=None, C=0.001, class_weight='balanced'):
    """the problems of a cross-validation: per group (in order of first appearance) and per fold value (sorted) the model trained on
    the group's rows of the other folds -> (jobs, costs): jobs a list of dict(group, fold, valid (row numbers), classes, lo, hi) with
    costs[lo:hi] its problems, costs (P, N) float32.  A group x fold without training or held-out rows has no job."""
    labels, folds = np.asarray(labels), np.asarray(folds)
    N = labels.shape[0]
    if folds.shape != (N,):
        raise ValueError("folds must be (N,) = (%d,), got %s" % (N, folds.shape))
    groups = np.zeros(N, np.int64) if groups is None else np.asarray(groups)
    if groups.shape != (N,):
        raise ValueError("groups must be (N,) = (%d,), got %s" % (N, groups.shape))
    _, first = np.unique(groups, return_index=True)
    jobs, blocks, lo = [], [], 0
    for g in groups[np.sort(first)]:
        in_g = groups == g
        for f in np.unique(folds[in_g]):
            valid, train = np.flatnonzero(in_g & (folds == f)), np.flatnonzero(in_g & (folds != f))
            if not len(valid) or not len(train):
                continue
            classes, costs = probe_costs(labels, train, C, class_weight)
            jobs.append(dict(group=g, fold=f, valid=valid, classes=classes, lo=lo, hi=lo + costs.shape[0]))
            blocks.append(costs)
            lo += costs.shape[0]
    return jobs, (np.concatenate(blocks, axis=0) if blocks else np.zeros((0, N), np.float32))


def cv_predictions(jobs, labels, dec):
    """held-out predictions and scores from the decisions dec (N, P) of every problem on every row -> dict(pred (N,) labels (rows
    that no job holds out keep their own label and count nowhere), scores {group: mean over its folds of the micro-F1, which is
    the accuracy}, mean: the mean over the groups, as the reference prints them)"""
    labels = np.asarray(labels)
    pred = labels.copy()
    per_group = {}
    for j in jobs:
        v = j['valid']
        pred[v] = labels_from_decision(j['classes'], dec[v, j['lo']:j['hi']])
        per_group.setdefault(j['group'], []).append(float(np.mean(pred[v] == labels[v])))
    scores = {g: float(np.mean(s)) for g, s in per_group.items()}
    return dict(pred=pred, scores=scores, mean=float(np.mean(list(scores.values()))) if scores else float('nan'))


def cross_validate(vae, z, labels, folds, groups=None, C=0.001, class_weight='balanced', tol=DEFAULT_TOL, max_newton=DEFAULT_MAX_NEWTON,
                   max_cg=DEFAULT_MAX_CG, return_parts=False):
    labels = _check_labels(z, labels)
    jobs, costs = cv_problems(labels, folds, groups, C, class_weight)
    if costs.shape[0] == 0:
        _check_fit_args(z, np.zeros((1, z.shape[0]), np.float32), tol, max_newton, max_cg)
        w, stats, dec = np.zeros((0, z.shape[1] + 1), np.float32), np.zeros((0, 4), np.float32), np.zeros((z.shape[0], 0), np.float32)
    else:
        w, stats = fit_raw(vae, z, costs, tol, max_newton, max_cg)
        dec = decision_raw(vae, z, w)
    res = cv_predictions(jobs, labels, dec)
    res['stats'] = stats
    if return_parts:
        res.update(jobs=jobs, costs=costs, w=w, decision=dec)
    return res
