"""The float64 restatement of SGD training that tests/test_gpu_sgd.py holds the step kernel to, as far as it can be checked without a
device -- and the reason that file exists.

Every other SGD training test of the suite runs ONE optimizer schedule: lam = 0.1, mu = 0.9, lr_decay = 0.95 with lr_step = 50, so that
below 51 epochs the learning rate is a constant.  Under that schedule a momentum hard-wired to 0.9 and an epoch whose first step takes
the previous epoch's learning rate change NOTHING (test_planted_errors_are_visible_off_the_default_schedule asserts a difference of
exactly 0), while under the other schedules of sgd_cases the same two errors stand hundreds to millions of times above a float32 run's
own distance from float64.  The step kernel's closed forms (closed_form_table in csrc/mf_job.h, engine.closed_form_scalars,
materialize_rows_kernel) are built from lr, lam and mu: a wrong one of them in any table, kernel argument or snapshot scalar passed
the suite before these two files.

Here: the restatement against torch.optim.SGD in float64, the conditions on the cases, the visibility of three planted errors, and
engine.closed_form_scalars against the restatement's rows without a rating."""
import numpy as np
import pytest
import torch

import sgd_cases as C
from ultrare_amd import engine


def torch_sgd(case, schedule):
    """torch.optim.SGD(momentum=mu, weight_decay=lam) on two dense float64 embeddings with MSELoss(sum), lam and mu at their float32
    values, the epoch's lr set in param_groups (as adam_cases.torch_adam does it): -> (U, V after the last epoch, loss [epochs])."""
    lam, mu = (float(np.float32(x)) for x in schedule[:2])
    lr_host = case.lr_of(schedule)
    U = torch.nn.Embedding(case.n_user, case.d, dtype=torch.float64)
    V = torch.nn.Embedding(case.n_item, case.d, dtype=torch.float64)
    with torch.no_grad():
        U.weight.copy_(torch.from_numpy(case.U0))
        V.weight.copy_(torch.from_numpy(case.V0))
    opt = torch.optim.SGD(list(U.parameters()) + list(V.parameters()), lr=float(lr_host[0]), momentum=mu, weight_decay=lam)
    loss_fn = torch.nn.MSELoss(reduction='sum')
    uid, iid = torch.from_numpy(case.uid.astype(np.int64)), torch.from_numpy(case.iid.astype(np.int64))
    r = torch.from_numpy(case.rating).double()
    losses = np.zeros(case.epochs)
    for e in range(case.epochs):
        for g in opt.param_groups:
            g['lr'] = float(lr_host[e])
        order = torch.from_numpy(case.orders[e].astype(np.int64))
        for s in range(case.steps):
            idx = order[s * case.B:(s + 1) * case.B]
            opt.zero_grad()
            loss = loss_fn((U(uid[idx]) * V(iid[idx])).sum(1), r[idx])
            loss.backward()
            opt.step()
            losses[e] += float(loss.detach())
    return U.weight.detach().numpy().copy(), V.weight.detach().numpy().copy(), np.sqrt(losses / case.N)


@pytest.mark.parametrize('schedule', [C.MIXED, C.NO_DECAY], ids=C.sid)
@pytest.mark.parametrize('case', [C.SHORT32, C.LONG16], ids=repr)
def test_restatement_equals_torch_sgd_in_float64(case, schedule):
    """float64 against float64: the two runs differ in the order of np.add.at's sums only."""
    U, V, loss = C.reference(case, schedule)['f64']
    Ut, Vt, loss_t = torch_sgd(case, schedule)
    assert np.abs(U[-1] - Ut).max() <= 1e-12 * np.abs(Ut).max() and np.abs(V[-1] - Vt).max() <= 1e-12 * np.abs(Vt).max()
    assert np.abs(loss / loss_t - 1.0).max() <= 1e-12


@pytest.mark.parametrize('case,schedule', C.PAIRS, ids=C.ids(C.PAIRS))
def test_every_case_and_schedule_is_well_behaved(case, schedule):
    """Conditions on the inputs, for the references alone: a pair that breaks them is replaced, not excused."""
    ref = C.reference(case, schedule)
    assert all(np.isfinite(x).all() for x in ref['f64'])
    assert ref['wmax'] <= 8
    assert all(np.isfinite(x).all() for x in ref['oracle']) and all(np.isfinite(x).all() for x in ref['f32'])
    print(f'{case!r} {schedule}: max|w| {ref["wmax"]:.3g} E_y {ref["E_y"]:.3g} (oracle {ref["E_y_oracle"][-1]:.3g}, float32 numpy '
          f'{ref["E_y_f32"][-1]:.3g}; per epoch ' + ' '.join(f'{x:.3g}' for x in ref['E_y_epoch']) + f') ulp32 {C.ulp32(ref["wmax"]):.3g}')
    assert np.isfinite(ref['E_y_epoch']).all() and min(ref['E_y_epoch']) > 0
    # the shape the cases are made for: rows without a rating on both sides, the last step of a short epoch partial
    assert case.uid.min() >= case.no_u == 5 and case.iid.min() >= case.no_i == 40 and np.bincount(case.iid)[-1] == case.N // 4


@pytest.mark.parametrize('case', C.SHORT + C.LONG, ids=repr)
def test_planted_errors_are_visible_off_the_default_schedule(case):
    """Three errors planted in the float64 restatement -- mu fixed at 0.9, the previous epoch's lr in an epoch's first step, rows that are
    not in an epoch's first batch skipping that step -- each stand, under the case's most telling schedule, at least 100 times above
    the bound 4 * max(E_y, ulp32(max|w|)) the GPU tests hold the kernel to.  Under the default schedule the first two change nothing at
    all: that is why this file and tests/test_gpu_sgd.py exist."""
    for plant in C.PLANTS:
        worst = 0.0
        for schedule in case.schedules:
            ref = C.reference(case, schedule)
            U, V, loss = C.ref_run(case, schedule, plant=plant)
            d = C.distance(ref, U[-1], V[-1], loss)
            if schedule == C.DEFAULT and plant != 'skip_first':
                assert d == 0.0, (plant, d)
            worst = max(worst, d / ref['bound'])
        print(f'{case!r} {plant}: {worst:.3g} x the bound at the most telling schedule')
        assert worst >= 100, (plant, worst)


SCALARS = [(c, s) for c in (C.SHORT32, C.LONG16, C.PAIR[0], C.UNEQUAL[0]) for s in c.schedules]


@pytest.mark.parametrize('case,schedule', SCALARS, ids=C.ids(SCALARS))
def test_closed_form_scalars_are_the_decay_of_a_row_without_a_rating(case, schedule):
    """engine.closed_form_scalars (the a_e of compact snapshots and of rows that only decay) against w_e / w_0 of such a row in the float64
    restatement, after every epoch: one rounding to float32 apart, 2 ulp32 allowed."""
    lam, mu = (float(np.float32(x)) for x in schedule[:2])
    a = engine.closed_form_scalars(case.lr_of(schedule), case.steps, lam, mu)
    assert a.dtype == np.float32 and a.shape == (case.epochs,)
    f64 = C.reference(case, schedule)['f64']
    for w0, w in ((case.U0[:case.no_u], f64[0][:, :case.no_u]), (case.V0[:case.no_i], f64[1][:, :case.no_i])):
        at = np.unravel_index(np.abs(w0).argmax(), w0.shape)
        assert abs(w0[at]) > 0.5
        ratio = w[(slice(None),) + at] / np.float64(w0[at])
        assert (np.abs(a.astype(np.float64) - ratio) <= 2 * np.spacing(np.abs(ratio).astype(np.float32))).all(), (a, ratio)
