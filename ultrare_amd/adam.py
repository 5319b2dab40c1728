"""The Adam optimizer of a training job (engine.TrainJob(..., optimizer='adam')) restated in numpy: what the owners of
csrc/mf_train.hip's mf_adam_step_kernel compute, as include/ultrare_hip.h states it (struct ure_shard: optimizer).

It is torch.optim.Adam(weight_decay=lam) -- the L2 term added to the gradient, dense over all rows, no amsgrad --:

    g  = acc + lam*w
    m' = m + c1*(g - m)                     c1 = 1 - beta1
    v' = beta2*v + (c2*g)*g                 c2 = 1 - beta2
    w' = w - s1[t] * ( m' / ( sqrt(v')/s2[t] + eps ) )

with s1[t] = lr(epoch of t) / (1 - beta1^(t+1)) and s2[t] = sqrt(1 - beta2^(t+1)) computed on the host in float64 -- as torch
computes its Python-float scalars -- and rounded to float32 once.  The kernel rounds every operation on its own and uses no fused
multiply-add, so adam_update_ref in float32 gives its bytes.  lam, beta1, beta2 and eps are float32 values everywhere (the
descriptor carries them so): betas32 / a float32 cast gives the numbers a job really runs with.
"""
import math

import numpy as np


def betas32(betas, eps):
    """(beta1, beta2, eps) as the Python floats of their float32 values: what the descriptor carries."""
    return float(np.float32(betas[0])), float(np.float32(betas[1])), float(np.float32(eps))


def _scalars64(lr_host, steps, beta1, beta2):
    out = np.empty((len(lr_host) * int(steps), 2), dtype=np.float64)
    t = 0
    for e in range(len(lr_host)):
        lr = float(lr_host[e])
        for _ in range(int(steps)):
            t += 1
            out[t - 1, 0] = lr / (1.0 - beta1 ** t)
            out[t - 1, 1] = math.sqrt(1.0 - beta2 ** t)
    return out


_SCALARS = {}


def adam_scalars(lr_host, steps, beta1, beta2):
    """float32 [epochs * steps, 2]: (s1[t], s2[t]) of every optimizer step of a shard with `steps` steps per epoch and the
    learning rate lr_host[e] in epoch e (struct ure_shard: opt_sc), from Python floats as torch makes them."""
    key = (np.asarray(lr_host, dtype=np.float64).tobytes(), int(steps), float(beta1), float(beta2))
    if key not in _SCALARS:
        if len(_SCALARS) > 64:
            _SCALARS.clear()
        _SCALARS[key] = _scalars64(lr_host, steps, float(beta1), float(beta2)).astype(np.float32)
    return _SCALARS[key].copy()


def adam_update_ref(w, m, v, acc, lam, beta1, beta2, eps, s1, s2):
    """One step of the rows w with moments m, v and data gradient acc (float32 arrays of one shape): -> (w', m', v'), every
    operation a float32 operation, in the kernel's order."""
    f = np.float32
    w, m, v, acc = (np.asarray(x, dtype=f) for x in (w, m, v, acc))
    lam, b1, b2, eps, s1, s2 = f(lam), f(beta1), f(beta2), f(eps), f(s1), f(s2)
    c1, c2 = f(1) - b1, f(1) - b2
    g = acc + lam * w
    m = m + c1 * (g - m)
    v = b2 * v + (c2 * g) * g
    den = np.sqrt(v) / s2 + eps
    return w - s1 * (m / den), m, v


def decay_rows_ref(w0, lr_host, steps, lam, betas=(0.9, 0.999), eps=1e-8):
    """The rows of a shard without interactions in it (acc = 0 in every step), from w0 and zero moments: -> per epoch (w, m, v)
    after its last step, float32, the bytes the kernel leaves."""
    b1, b2, eps = betas32(betas, eps)
    sc = adam_scalars(lr_host, steps, b1, b2)
    w = np.asarray(w0, dtype=np.float32).copy()
    m, v, zero, out = np.zeros_like(w), np.zeros_like(w), np.zeros_like(w), []
    for t in range(len(sc)):
        w, m, v = adam_update_ref(w, m, v, zero, lam, b1, b2, eps, sc[t, 0], sc[t, 1])
        if (t + 1) % int(steps) == 0:
            out.append((w.copy(), m.copy(), v.copy()))
    return out


def adam_train_ref(uid, iid, rating, U0, V0, orders, batch, lr_host, lam, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
    """Whole training of one shard, dense: epoch e takes the batches orders[e][s*batch:(s+1)*batch] (read.py:133), the loss is the
    summed squared error (MSELoss(sum)), the L2 term lam*w goes into the gradient of EVERY row, then Adam.  lam, betas, eps are
    taken at their float32 values (betas32); dtype float64 computes the scalars and everything else in double, float32 uses
    adam_scalars and adam_update_ref.
    -> (U, V, loss [epochs] = the epoch's summed squared errors, gmin_U, gmin_V = per element the smallest |g| of any step)."""
    uid, iid = np.asarray(uid, dtype=np.int64), np.asarray(iid, dtype=np.int64)
    r = np.asarray(rating, dtype=np.float32).astype(dtype)
    W = [np.asarray(U0, dtype=dtype).copy(), np.asarray(V0, dtype=dtype).copy()]
    M, S = [np.zeros_like(x) for x in W], [np.zeros_like(x) for x in W]
    gmin = [np.full(x.shape, np.inf) for x in W]
    b1, b2, eps = betas32(betas, eps)
    lam = float(np.float32(lam))
    steps = (len(r) + batch - 1) // batch
    sc = adam_scalars(lr_host, steps, b1, b2) if dtype == np.float32 else _scalars64(lr_host, steps, b1, b2)
    loss, t = np.zeros(len(lr_host), dtype=np.float64), 0
    for e in range(len(lr_host)):
        order = np.asarray(orders[e], dtype=np.int64)
        for s in range(steps):
            idx = order[s * batch:(s + 1) * batch]
            u, i = uid[idx], iid[idx]
            err = np.sum(W[0][u] * W[1][i], axis=1, dtype=dtype) - r[idx]
            loss[e] += float(np.sum(err.astype(np.float64) ** 2))
            acc = [np.zeros_like(W[0]), np.zeros_like(W[1])]
            ge = (2 * err)[:, None]
            np.add.at(acc[0], u, ge * W[1][i])
            np.add.at(acc[1], i, ge * W[0][u])
            for k in range(2):
                g = acc[k] + dtype(lam) * W[k]
                gmin[k] = np.minimum(gmin[k], np.abs(g))
                if dtype == np.float32:
                    W[k], M[k], S[k] = adam_update_ref(W[k], M[k], S[k], acc[k], lam, b1, b2, eps, sc[t, 0], sc[t, 1])
                else:
                    M[k] = M[k] + (1.0 - b1) * (g - M[k])
                    S[k] = b2 * S[k] + ((1.0 - b2) * g) * g
                    W[k] = W[k] - sc[t, 0] * (M[k] / (np.sqrt(S[k]) / sc[t, 1] + eps))
            t += 1
    return W[0], W[1], loss, gmin[0], gmin[1]
