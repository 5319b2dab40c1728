"""The learned shard combiner, host side: the Newton fit of at most 33 unknowns from the sufficient
statistics the device leaves (engine.combine_stats / ure_combine_stats), and the fitted object the scoring path takes.

The reference's third SISA stage is the plain mean of the shard scores (method/utils.py:140-145).  Here a generalised
linear model z = b + sum_s w[s] p_s over the S shard scores of a pair is fitted to the training ratings, one weight row per
user group or one for all; link 'linear' predicts z, link 'logistic' predicts sigmoid(z) against the soft target r in [0, 1].
The ridge pulls w towards 1/S, so l2 -> inf with the linear link is the mean ensemble again.  Nothing here touches the
device: the fit is written against a function `stats(theta) -> float64 vector`, which the tests feed from numpy.
"""
import numpy as np

LINKS = {'linear': 0, 'logistic': 1}
MAX_MODELS = 32          # URE_MAX_MODELS_PER_CALL
MAX_HALVINGS = 30        # of one Newton step before the fit stops where it is


def stats_len(S):
    """Doubles of a stats vector: n, loss, g [S + 1], upper triangle of H [(S + 1)(S + 2) / 2]."""
    return 2 + (S + 1) + (S + 1) * (S + 2) // 2


def unpack_stats(v, S):
    """-> (n, loss, g [S + 1], H [S + 1, S + 1] symmetric) of a stats vector."""
    v = np.asarray(v, dtype=np.float64)
    X = S + 1
    if v.shape != (stats_len(S),):
        raise ValueError(f'a stats vector of {S} models has {stats_len(S)} entries, not {v.shape}')
    H = np.zeros((X, X))
    H[np.triu_indices(X)] = v[2 + X:]
    H = H + np.triu(H, 1).T
    return int(round(v[0])), float(v[1]), v[2:2 + X].copy(), H


def link_code(link):
    if isinstance(link, str) and link in LINKS:
        return LINKS[link]
    raise ValueError(f"link must be 'linear' or 'logistic', not {link!r}")


def check_fit_args(link, l2, max_iter, tol):
    """The fit's settings, checked before any device work (ValueError) -> the link's code."""
    code = link_code(link)
    if isinstance(l2, bool) or not isinstance(l2, (int, float, np.floating, np.integer)) or not (np.isfinite(l2) and l2 >= 0):
        raise ValueError(f'l2 must be a finite number >= 0, not {l2!r}')
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f'max_iter must be an integer >= 1, not {max_iter!r}')
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.floating, np.integer)) or not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f'tol must be a finite number >= 0, not {tol!r}')
    return code


def mean_weights(S):
    """The start point and the ridge's centre: the mean ensemble, w = 1/S, b = 0."""
    return np.concatenate([np.full(S, 1.0 / S), [0.0]])


def newton_fit(stats, S, link, l2=0.0, max_iter=25, tol=1e-10):
    """Minimise loss(theta) + (l2 / 2) |w - 1/S|^2 over theta = (w [S], b) from the mean start.  stats(theta) -> the stats
    vector of the pair set at theta (one pass over the data per call).  Newton steps delta = solve(H + l2 diag(1..1, 0),
    g + l2 (w - 1/S, 0)), each halved while the objective does not decrease (a pass per trial), until max |delta| <= tol
    or max_iter accepted steps.  The linear link is quadratic: one step, then the pass that accepted it is the final one.
    -> dict: theta, n, iters, loss_before, loss_after, grad_norm (max |g + penalty| at theta), objective (the accepted
    values, non-increasing), passes (calls of stats)."""
    code = check_fit_args(link, l2, max_iter, tol)
    centre = mean_weights(S)
    mask = np.concatenate([np.ones(S), [0.0]])
    passes = [0]

    def at(theta):
        passes[0] += 1
        n, loss, g, H = unpack_stats(stats(theta), S)
        pen = theta - centre
        return {'n': n, 'loss': loss, 'obj': loss + 0.5 * l2 * float(np.sum(mask * pen * pen)), 'grad': g + l2 * mask * pen,
                'hess': H + l2 * np.diag(mask)}

    def bad(what):
        return ValueError(f'fit_combiner: {what} with l2 = {l2:g}: the shard scores are collinear (or not finite) on these '
                          f'pairs; a larger l2 makes the system definite')
    theta = centre.copy()
    cur = at(theta)
    if not (np.isfinite(cur['obj']) and np.isfinite(cur['grad']).all() and np.isfinite(cur['hess']).all()):
        raise bad('non-finite statistics at the mean start')
    loss_before, objective, iters = cur['loss'], [cur['obj']], 0
    while iters < max_iter:
        try:
            delta = np.linalg.solve(cur['hess'], cur['grad'])
        except np.linalg.LinAlgError:
            raise bad('singular Newton system') from None
        # a solve that did not solve: the system is singular to working precision
        scale = np.abs(cur['hess']) @ np.abs(delta) + np.abs(cur['grad'])
        if not np.isfinite(delta).all() or (np.abs(cur['hess'] @ delta - cur['grad']) > 1e-6 * scale + 1e-300).any():
            raise bad('singular Newton system')
        if np.abs(delta).max() <= tol:
            break
        step, nxt = 1.0, None
        for _ in range(MAX_HALVINGS):
            trial = at(theta - step * delta)
            if np.isfinite(trial['obj']) and trial['obj'] < cur['obj']:
                nxt = trial
                break
            step *= 0.5
        if nxt is None:          # no shorter step decreases the objective: theta is the minimiser to rounding
            break
        theta, cur = theta - step * delta, nxt
        iters += 1
        objective.append(cur['obj'])
        if code == 0:
            break
    if not np.isfinite(cur['grad']).all():
        raise bad('non-finite statistics at the fitted point')
    return {'theta': theta, 'n': cur['n'], 'iters': iters, 'loss_before': loss_before, 'loss_after': cur['loss'],
            'grad_norm': float(np.abs(cur['grad']).max()), 'objective': objective, 'passes': passes[0]}


def first_group_map(groups, n_user):
    """group_of_user int32 [n_user]: the FIRST group that lists the user (the rule of Sisa.unlearn, sisa.py:76-81), -1 for
    a user in no group.  Ids outside [0, n_user) are an error."""
    out = np.full(int(n_user), -1, dtype=np.int32)
    for g in reversed(range(len(groups))):
        idx = np.asarray(groups[g], dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n_user):
            raise ValueError(f'group {g} lists user ids outside [0, {n_user})')
        out[idx] = g
    return out


class Combiner:
    """Fitted weights of the shard scores.  W float64 [G, S + 1] (host; row g = (w, b) of group g), link ('linear' |
    'logistic'), groups (the index lists the rows belong to, or None: one row for every user), and per group n, iters,
    loss_before (at the mean start), loss_after, grad_norm."""

    def __init__(self, W, link, groups=None, n=None, iters=None, loss_before=None, loss_after=None, grad_norm=None):
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] < 2 or W.shape[1] - 1 > MAX_MODELS or not np.isfinite(W).all():
            raise ValueError(f'W must be a finite [G, S + 1] array with 1 <= S <= {MAX_MODELS}, not {W.shape}')
        if groups is None and W.shape[0] != 1:
            raise ValueError(f'{W.shape[0]} weight rows need the groups they belong to')
        if groups is not None and len(groups) != W.shape[0]:
            raise ValueError(f'{W.shape[0]} weight rows for {len(groups)} groups')
        self.W, self.link, self.groups = W, link, groups
        self.link_code = link_code(link)
        G = W.shape[0]
        fill = lambda v, dt: np.zeros(G, dtype=dt) if v is None else np.asarray(v, dtype=dt)
        self.n, self.iters = fill(n, np.int64), fill(iters, np.int64)
        self.loss_before, self.loss_after, self.grad_norm = fill(loss_before, np.float64), fill(loss_after, np.float64), fill(grad_norm, np.float64)
        self._dev = {}

    @property
    def n_models(self):
        return self.W.shape[1] - 1

    def group_of_user(self, n_user):
        """int32 [n_user] (None without groups).  A user in no group takes the mean ensemble under the linear link and is
        an error under the logistic one, where the mean of the scores is not a prediction."""
        if self.groups is None:
            return None
        m = first_group_map(self.groups, n_user)
        if self.link_code != 0 and (m < 0).any():
            raise ValueError(f"{int((m < 0).sum())} of {n_user} users are in no group (the first: {int(np.flatnonzero(m < 0)[0])}): "
                             "link='logistic' has no weights for them")
        return m

    def on_device(self, device, n_user):
        """(W tensor [G, S + 1] float64, group_of_user int32 tensor or None) on `device`, uploaded once per (device, n_user)."""
        import torch
        key = (str(device), int(n_user))
        if key not in self._dev:
            m = self.group_of_user(n_user)
            self._dev[key] = (torch.from_numpy(self.W).to(device), None if m is None else torch.from_numpy(m).to(device))
        return self._dev[key]

    def __repr__(self):
        return f'Combiner(link={self.link!r}, G={self.W.shape[0]}, S={self.n_models}, n={self.n.tolist()}, iters={self.iters.tolist()})'
