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


# ---------------------------------------------------------------------------------------------------------------------
# Ranking under the fitted weights (csrc/mf_combine_rank.hip, include/ultrare_combine_rank.h): the contract in numpy.
# ---------------------------------------------------------------------------------------------------------------------
def weight_rows(W, users, group_of_user=None):
    """The weight row of every user of `users` -> (rows float64 [n, S + 1], outside bool [n]): W[group_of_user[u]], row 0
    without a map; a user whose entry is outside [0, G) (or whose id is outside the map) is `outside` and gets the mean
    ensemble w = 1/S, b = 0."""
    W = np.asarray(W, dtype=np.float64)
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    if group_of_user is None:
        g = np.zeros(len(users), dtype=np.int64)
    else:
        m = np.asarray(group_of_user, dtype=np.int64)
        inside = (users >= 0) & (users < len(m))
        g = np.where(inside, m[np.where(inside, users, 0)], -1)
    outside = (g < 0) | (g >= len(W))
    rows = W[np.where(outside, 0, g)].copy()
    rows[outside] = mean_weights(W.shape[1] - 1)
    return rows, outside


def weighted_scores_ref(P, link, rows, outside=None):
    """score_w of ure_score_weighted from the per-model float32 scores P [n, S] (column s: model s's score as ure_score gives
    it for that model alone) and the pairs' weight rows [n, S + 1]: p_s = 0.f + P[:, s] (a score of -0.0 becomes +0.0);
    z = b, then z = z + w[s] * (double)p_s for s = 0, 1, ... with every product rounded; mu = z (link 0) or
    1 / (1 + exp(-z)) (link 1); -> (float32)mu.  `outside` pairs (weight_rows) are NaN under link 1.  numpy's exp may differ
    from the device's in the last place: the linear link is exact here, the logistic one to that."""
    code = link if isinstance(link, (int, np.integer)) and not isinstance(link, bool) else link_code(link)
    P = np.asarray(P, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.float64)
    S = P.shape[1]
    z = rows[:, S].copy()
    for s in range(S):
        z = z + rows[:, s] * (np.float32(0) + P[:, s]).astype(np.float64)
    with np.errstate(over='ignore'):
        mu = z if code == 0 else 1.0 / (1.0 + np.exp(-z))
    if code != 0 and outside is not None:
        mu = np.where(outside, np.nan, mu)
    return mu.astype(np.float32)


def recommend_ref(scores, top_k, excl=None):
    """ure_recommend_topk_weighted over a score matrix [n, n_item] float32 (score_w of every (query user, item) pair) ->
    (scores [n, top_k] float32, items [n, top_k] int64): per query row the top_k non-excluded items in key order (score
    descending, NaN below -inf, -0.0 == +0.0, then item id ascending); padding is (NaN, -1).  excl = (off [n + 1], items)."""
    from .nmf import recommend_ref as by_key
    scores = np.asarray(scores, dtype=np.float32)
    return by_key(None, None, None, None, scores.shape[1], top_k, excl, scores=scores)


def rank_ref(scores, targets, excl=None):
    """ure_rank_pairs_weighted over a score matrix [n, n_item] float32 -> ranks int32 [n_targets] in input order: for target t
    of query row q the number of non-excluded items whose key beats t's, -1 when t is excluded.  targets = (off [n + 1],
    items): any order, duplicates, empty rows.  A target of rank r < top_k is item r of recommend_ref's row."""
    from .nmf import rank_ref as by_key
    scores = np.asarray(scores, dtype=np.float32)
    return by_key(None, None, None, None, targets, excl, scores=scores, n_item=scores.shape[1])


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

    def check_query(self, n_models, users, n_user):
        """What recommend / rank_eval check before any device work (ValueError): the combiner was fitted on n_models models, and
        under the logistic link every QUERY user is in a group (under the linear link such a user takes the mean weights)."""
        if self.n_models != n_models:
            raise ValueError(f'the combiner was fitted on {self.n_models} models, not {n_models}')
        if self.groups is None or self.link_code == 0:
            return
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        m = first_group_map(self.groups, n_user)
        lost = users[(users < 0) | (users >= n_user) | (m[np.clip(users, 0, max(n_user - 1, 0))] < 0)] if n_user > 0 else users
        if lost.size:
            raise ValueError(f"{lost.size} of {users.size} query users are in no group (the first: {int(lost[0])}): link='logistic' has no weights for them")

    def on_device_for_query(self, device, n_user):
        """on_device for a ranking call: the same tensors, but the map is not refused for users outside every group (check_query
        has looked at the query users; the others are not scored)."""
        import torch
        key = (str(device), int(n_user), 'query')
        if key not in self._dev:
            m = None if self.groups is None else first_group_map(self.groups, n_user)
            self._dev[key] = (torch.from_numpy(self.W).to(device), None if m is None else torch.from_numpy(m).to(device))
        return self._dev[key]

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
