"""The bytes of the attribute probe's kernels (csrc/attack.hip, csrc/adv.hip, csrc/probe.h) pinned to a recording: cases only, shared by
tests/test_gpu_attack.py::test_probe_bytes_are_the_recorded_ones and tests/golden/make_golden_probe.py, which wrote
tests/golden/probe_parent_bytes.json on an MI355X from the library of the commit BEFORE the two files shared probe.h.  The float32
yardstick of the other tests would not notice a refactor that changed a chain's order; this does.

A case is (H, d, m, folds), everything through the C ABI on seeded numpy inputs, unsorted rows of a wider NaN-filled table:
  (H, d)   every HQ / DQ quarter boundary of attack_train_kernel<HQ, DQ> (16 | 17, 64 | 65, and 7 / 31 / 33 between), an odd He and a
           d + 1 that is a multiple of 32 (the two row-stride cases of adv_input_grad_kernel), and both limits (0 / 1 and 128)
  m        773 (three chunks and a tail of 5) and 2 folds (the minimum)
  folds    2 and 5
  trained  two epochs of ure_attack_standardize + ure_attack_train (the second reads the first's moments): params, loss and the chunk
           sums of the last epoch out of the scratch (test_gpu_attack._train_raw's view)
  probed   on adv_cases.probe's untrained inputs: ure_attack_score's scores, ure_adv_input_grad's grad and p for both targets
"""
import hashlib

import numpy as np

import adv_cases as D

SHAPES = ((0, 17), (1, 1), (7, 31), (16, 16), (17, 33), (64, 64), (65, 128), (128, 128))
CASES = tuple((H, d, m, folds) for H, d in SHAPES for folds in (2, 5) for m in (773, 2 * folds))
TARGETS = ((0.5, 0.5), (0.0, 1.0))
EPOCHS = 2


def name(case):
    return 'H{}_d{}_m{}_f{}'.format(*case)


def wide(x, ld, seed):
    """tests/test_gpu_attack.py's construction: the rows of x at an unsorted selection of a NaN-filled table [2 m + 7, ld]."""
    m, d = x.shape
    rows = np.random.RandomState(seed).permutation(2 * m + 7)[:m]
    W = np.full((2 * m + 7, ld), np.nan, dtype=np.float32)
    W[rows, :d] = x
    return W, rows


def train_inputs(case):
    """(W, rows, n1, fold_of, params0) of test_gpu_attack.test_one_epoch_from_given_parameters' kind: biases off zero."""
    from ultrare_amd import attack as A
    H, d, m, folds = case
    rs = np.random.RandomState(100000 * H + 1000 * d + 10 * folds + (m > 100))
    n1 = max(folds, m // 3)
    x = rs.randn(m, d).astype(np.float32)
    x[:n1] += np.float32(0.5)
    W, rows = wide(x, d + 3, m + d)
    fold_of = A.fold_plan(n1, m - n1, folds, H + d)
    p0 = (A.init_params(d, H, folds, H + d) + rs.uniform(-0.05, 0.05, (folds, A.n_params(d, H)))).astype(np.float32)
    return W, rows, n1, fold_of, p0


def probed(nv, case):
    """{name: array} of the score and input-gradient entries on adv_cases.probe(m, d, H, folds)."""
    import torch
    from ultrare_amd import adv_unlearn as V
    H, d, m, folds = case
    c = D.probe(m, d, H, folds, 7000 + 100 * H + d + folds)
    W, rows = wide(c['x'], d + 3, m + d)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    perm, off = V.fold_groups(c['fold_of'], folds)
    Wt, rows_d, fo, params, stats, fw, perm_d, off_d = [up(a) for a in (W, rows.astype(np.int32), c['fold_of'], c['params'], c['stats'], c['fw'], perm, off)]
    L, st = nv.lib(), nv.stream_handle(None)
    scores = torch.empty(m, dtype=torch.float32, device='cuda')
    nv.check(L.ure_attack_score(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), fo.data_ptr(), m, folds, H, stats.data_ptr(), params.data_ptr(),
                                scores.data_ptr(), st), 'ure_attack_score')
    out = {'scores': scores}
    for t0, t1 in TARGETS:
        grad, p = torch.empty(m, d, dtype=torch.float32, device='cuda'), torch.empty(m, dtype=torch.float32, device='cuda')
        nv.check(L.ure_adv_input_grad(Wt.data_ptr(), Wt.stride(0), d, rows_d.data_ptr(), fo.data_ptr(), m, c['n1'], folds, H, stats.data_ptr(),
                                      params.data_ptr(), fw.data_ptr(), t0, t1, grad.data_ptr(), p.data_ptr(), perm_d.data_ptr(), off_d.data_ptr(), st),
                 'ure_adv_input_grad')
        out[f'grad_{t0:g}_{t1:g}'], out[f'p_{t0:g}_{t1:g}'] = grad, p
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def digests(nv, train_raw, case):
    """{name: sha256 of the array's bytes} of one case; train_raw is tests/test_gpu_attack.py's _train_raw."""
    H, d, m, folds = case
    W, rows, n1, fold_of, p0 = train_inputs(case)
    params, loss, sums = train_raw(nv, W, d, rows, n1, fold_of, p0, H, EPOCHS, 1e-2, 1e-3)
    arrays = {'params': params, 'loss': loss, 'chunk_sums': sums, **probed(nv, case)}
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in arrays.items()}
