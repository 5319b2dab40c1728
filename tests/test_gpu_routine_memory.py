"""The later backbones' jobs and the device routines composed in Python, on poisoned memory (the job's rule read for a
composition: every byte a launch reads was uploaded by the routine or written by an earlier launch of the same call).

tests/test_gpu_job_memory.py runs TrainJob, Adam, one MSE GcnJob and one MF request this way; this module does it for what was
added since.  A case builds its inputs once on the host, outside the poison; inside poison.active(monkeypatch, fill) it runs the
routine and collects every byte a caller can obtain as {name: numpy array} -- the device logs and flags too, and for a routine that
works in place the whole table, not only the rows it names.  The fill varies fastest, 0x00 first: that run is held to the reference
the family's own test module holds the routine to (the same helper, the same bound; no tolerance is introduced here), every other
run -- 0xFF, 0x5A and one without the helper -- to the 0x00 run, array by array, through test_gpu_job_memory.differences.

The cases (the smallest shapes at which the routine still has the structure that can go wrong), and the seconds one parametrised
test of each took on an MI355X: the 0x00 run with its reference (the first of a process also loads the library), then the slowest of
the other three fills:
  B1, B2   2.19 / 0.04, 0.04 / 0.01   GcnJob(loss='bpr'): bpr_cases.WHOLE_STEP_CASES[0] and the layers = 0 one
  A1, A2   0.08 / 0.01, 0.07 / 0.01   GcnJob(attr=...) d2d and u2u, two epochs, four steps of the first skipped
           (B1 .. A2 exercise the reference bar only: a GcnJob draws every buffer from torch.zeros and none from the library's block
           cache, so no fill reaches what it reads and these sixteen tests cannot fail on a read-before-write inside the job -- a buffer
           that epoch e reads and only epoch e - 1 wrote is hidden equally.  What they keep is that it stays so: a buffer moved to
           torch.empty would bring the job into INVENTORY and under the fills.  L1 runs the same kernels on torch.empty memory.)
  K1       0.59 / 0.01   attack_fit + auc_counts + confusion_counts + attack_scores: the hidden layer and the logistic probe, two epochs
  V1       0.31 / 0.01   adversarial_unlearn, adv_cases.SHORT, on the current and on a side stream
  N1       2.05 / 0.04   inf_solve (case A: gn, damped full, out of iterations; case C: gn), inf_matvec, newton_unlearn of two steps on case C
  R1       1.28 / 0.01   als_sweeps (one and two sweeps), fold_in against one table and against the mean
  R2       0.08 / 0.01   wmf_sweeps (l2_n = 0 and 0.02; one and two sweeps), wmf_fold_in
  C1       1.52 / 0.04   ot_cluster: exact and Sinkhorn, CSR rows (crafted('columns')) and dense rows (the toy embedding)
  C2       0.31 / 0.01   kmeans(balanced=True) on the CSR and on the dense route, n_init = 2, max_iter = 3
  C3       1.16 / 0.02   kmedoids on the given array of tests/golden/cluster_toy.npz and streamed from sparse rows
  C4       0.09 / 0.02   singleLPA / lpa on the same two sources
  C5       0.21 / 0.01   findNeighbor, dense and sparse rows, the cache file included
  S1       1.4 / 0.03    fit_combiner (both links, per group), recommend, rank_eval and baseTest with and without it
  S2       0.71 / 0.01   recommend_nmf, rank_eval_nmf
  U1       0.24 / 0.01   attribute_unlearn d2d and u2u, three steps
  Q1, Q2   0.88 / 0.03, 0.79 / 0.02   a Sisa request of three shards: 'lightgcn' with loss='bpr', and 'wmf': learn, then unlearn of shard 1
  Q3       0.91 / 0.08   the MF request of tests/test_gpu_surface.py with the batch tags made on the host (URE_DEVICE_TAGS=0), both modes
  L1       0.03 / 0.01   the stateless step calls: gcn_step_tags, gcn_propagate, gcn_loss_grad, bpr_negatives, bpr_neg_index, bpr_loss_grad
and 0.01 for each of the two planted-buffer tests.

INVENTORY classifies every function of ultrare_amd/ that draws uninitialised memory (torch.empty, torch.empty_like, Tensor.new_empty):
tests/test_cpu_poison_inventory.py fails for a new one that nobody classified.  A 'routine' claim is checked here: the 0x00 run of
every case records which of these functions allocated through the poisoned torch.empty, and the case must have reached every name
the table credits to it."""
import ast
import os
import sys
import time

import numpy as np
import pytest
import torch

import adv_cases
import attack_cases
import attr_train_cases
import bpr_cases
import influence_cases
import nmf_cases
import poison
import wmf_cases
from test_gpu_job_memory import FILL_IDS, FILLS, differences

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, 'golden')
PKG = os.path.join(os.path.dirname(HERE), 'ultrare_amd')
ULP32 = 2.0 ** -24


# ================================================================== the inventory of uninitialised allocations
def allocating_functions(root=PKG):
    """-> ({'module:qualname': [line, ...]} of every function or method under `root` whose body names torch.empty, torch.empty_like or
    .new_empty -- a lambda or a comprehension counts for the def around it --, {file: [(first, last, 'module:qualname', is_fake)]} of
    every def, for looking a frame up)."""
    found, spans = {}, {}
    for folder, _, files in sorted(os.walk(root)):
        for f in sorted(files):
            if not f.endswith('.py'):
                continue
            path = os.path.join(folder, f)
            module = os.path.relpath(path, root)[:-3].replace(os.sep, '.')
            with open(path) as fh:
                tree = ast.parse(fh.read())
            spans[os.path.realpath(path)] = here = []

            def visit(node, qual):
                for child in ast.iter_child_nodes(node):
                    if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        name = f"{module}:{'.'.join(qual + [child.name])}"
                        first = min([child.lineno] + [d.lineno for d in child.decorator_list])
                        fake = any(isinstance(d, ast.Attribute) and d.attr == 'register_fake' for d in child.decorator_list)
                        here.append((first, child.end_lineno, name, fake))
                        visit(child, qual + [child.name])
                    elif isinstance(child, ast.ClassDef):
                        visit(child, qual + [child.name])
                    else:
                        if isinstance(child, ast.Attribute) and (child.attr == 'new_empty' or (
                                child.attr in ('empty', 'empty_like') and isinstance(child.value, ast.Name) and child.value.id == 'torch')):
                            found.setdefault(f"{module}:{'.'.join(qual) or '<module>'}", []).append(child.lineno)
                        visit(child, qual)
            visit(tree, [])
    return found, spans


def function_at(spans, filename, line):
    """The innermost def of `filename` that holds `line`, or None."""
    best = None
    for first, last, name, _ in spans.get(os.path.realpath(filename), ()):
        if first <= line <= last and (best is None or first >= best[0]):
            best = (first, name)
    return best and best[1]


def watch(monkeypatch, seen, spans):
    """Beside the poison: count, by the calling frame's function, who draws uninitialised memory; `seen` receives the names."""
    for owner, name in ((torch, 'empty'), (torch, 'empty_like'), (torch.Tensor, 'new_empty')):
        inner = getattr(owner, name)

        def counted(*args, _inner=inner, **kw):
            frame = sys._getframe(1)
            who = function_at(spans, frame.f_code.co_filename, frame.f_lineno)
            if who is not None:
                seen.add(who)
            return _inner(*args, **kw)
        monkeypatch.setattr(owner, name, counted)


_JOB = 'tests/test_gpu_job_memory.py::test_a_job_gives_the_same_bytes_on_memory_of_every_fill'
_REQUEST = 'tests/test_gpu_job_memory.py::test_a_request_gives_the_same_bytes_on_memory_of_every_fill'
_NMF_JOB = 'tests/test_gpu_nmf.py::test_job_on_poisoned_memory'
_NMF_SCORE = 'tests/test_gpu_nmf.py::test_scoring_equals_the_contract'
_SERIES = 'tests/test_gpu_score_contract.py::test_series_routes_equal_single_evaluations_at_every_width'
_ARENA = 'tests/test_gpu_abi_memory.py::test_entry_keeps_the_memory_contract'
_GCN = 'tests/test_gpu_lightgcn.py::test_every_entry_keeps_the_memory_contract_on_dirty_memory'
_BPR = 'tests/test_gpu_bpr.py::test_every_entry_keeps_the_memory_contract_on_dirty_memory'
_SEL = 'tests/test_gpu_attr_train.py::test_the_selection_entries_keep_the_memory_contract_on_dirty_memory'
_DEV = 'tests/test_gpu_attr_train.py::test_device_counted_losses_stay_inside_the_derived_bounds_on_dirty_memory'
_ADV = 'tests/test_gpu_adv.py::test_the_entry_on_dirty_memory_inside_guard_zones'
_SCORE = 'tests/test_gpu_score_contract.py::test_score_equals_the_contract_at_every_width_count_and_model_count'

CLASSES = ('routine', 'job', 'entry', 'meta', 'host', 'collective')
# 'routine': the cases of this module whose run() reaches it (checked in the 0x00 run).  'job': a whole job or request on poisoned memory
# elsewhere.  'entry': a plain wrapper of one raw entry whose outputs come straight from that entry; the note is its guard-zone test.
# 'meta': shape-only registrations.  'host': CPU or pinned memory that one call overwrites whole before anything reads it; the note
# names the call.  'collective': the receive buffers of ONE collective among several ranks, which no single-GPU case can run: the
# call writes them whole; the note names it.
INVENTORY = {
    # ---- engine.py: the training job, the evaluation sets
    'engine:LayoutPlan.__init__': ('job', _REQUEST), 'engine:LayoutPlan.allocate': ('job', _JOB),
    'engine:TrainJob._allocate_pools': ('job', _JOB), 'engine:TrainJob.own_scores': ('entry', _SERIES),
    'engine:TrainJob.epoch_sse_queue': ('job', _JOB), 'engine:ScoreCache.base': ('job', _REQUEST),
    'engine:EvalSet.__init__': ('routine', 'S1 Q1 Q2'), 'engine:EvalSet._series_buffers': ('job', _REQUEST),
    'engine:EvalSet.score_vector': ('job', _REQUEST),
    # ---- ranking, recommendation, the combiner
    'engine:recommend': ('routine', 'S1'), 'engine:rank_pairs': ('routine', 'S1'), 'engine:combine_stats': ('routine', 'S1'),
    'engine:score_weighted': ('entry', _ARENA),
    # ---- the pair-distance reductions, Sinkhorn, the CSR kernels
    'engine:pair_knn': ('routine', 'C5'), 'engine:pair_rowsum': ('routine', 'C3'), 'engine:pair_cols': ('routine', 'C3'),
    'engine:pair_label_expsum': ('routine', 'C4'), 'engine:ot_sinkhorn': ('routine', 'C1'),
    'engine:_csr_cost_call': ('routine', 'C1 C2'), 'engine:csr_centroids': ('routine', 'C1'),
    'engine:csr_kmeans_centroids': ('routine', 'C2'), 'engine:balanced_fill': ('routine', 'C2'),
    # ---- ridge and WMF
    'engine:ridge_rows': ('routine', 'R1'), 'engine:gram': ('routine', 'R2'), 'engine:wridge_rows': ('routine', 'R2'),
    # ---- attribute unlearning, the attacker, the adversarial loop
    'engine:_attr_scratch': ('routine', 'U1'), 'engine:mmd_bandwidth': ('routine', 'U1'), 'engine:mmd_loss_grad': ('routine', 'U1'),
    'engine:u2u_loss_grad': ('routine', 'U1'), 'engine:mmd_matrix': ('entry', _ARENA),
    'engine:attack_fit': ('routine', 'K1'), 'engine:_ProbeRun.__init__': ('routine', 'K1 V1'), 'engine:attack_input_grad': ('entry', _ADV),
    'engine:adversarial_unlearn': ('routine', 'V1'), 'engine:attack_scores': ('routine', 'K1'), 'engine:auc_counts': ('routine', 'K1'),
    'engine:confusion_counts': ('routine', 'K1'),
    # ---- LightGCN, BPR, the per-batch attribute term: the jobs draw zeros; these are the stateless calls beside them
    'engine:gcn_propagate': ('routine', 'L1'), 'engine:gcn_step_tags': ('routine', 'L1'), 'engine:gcn_loss_grad': ('routine', 'L1'),
    'engine:bpr_negatives': ('routine', 'L1'), 'engine:bpr_neg_index': ('routine', 'L1'), 'engine:bpr_loss_grad': ('routine', 'L1'),
    'engine:attr_step_masks': ('entry', _SEL), 'engine:attr_select': ('entry', _SEL), 'engine:mmd_loss_grad_dev': ('entry', _DEV),
    'engine:u2u_loss_grad_dev': ('entry', _DEV),
    # ---- NeuMF
    'engine:nmf_score': ('entry', _NMF_SCORE), 'engine:nmf_recommend': ('routine', 'S2'), 'engine:nmf_rank_pairs': ('routine', 'S2'),
    'engine:NmfJob.__init__': ('job', _NMF_JOB),
    # ---- influence
    'engine:inf_coef': ('routine', 'N1'), 'engine:inf_matvec': ('routine', 'N1'), 'engine:inf_grad': ('routine', 'N1'),
    'engine:inf_dot': ('routine', 'N1'), 'engine:inf_objective': ('routine', 'N1'), 'engine:inf_solve': ('routine', 'N1'),
    # ---- measure.py, ops.py
    'measure:ot_request': ('entry', _ARENA),
    'ops:mf_score': ('entry', _SCORE), 'ops:_': ('meta', 'register_fake'), 'ops:_cost': ('entry', _ARENA), 'ops:ot_centroids': ('entry', _ARENA),
    'ops:gcn_propagate': ('entry', _GCN), 'ops:bpr_negatives': ('entry', _BPR),
    # ---- rng.py: host draws, staging, the device shuffle of a request
    'rng:native_fill_ok': ('host', 'Tensor.normal_ / random_ and ure_host_mf_init fill every element'),
    'rng:device_fill_ok': ('host', 'Tensor.normal_ / random_ fill every element'),
    'rng:mf_init_device': ('entry', _ARENA),
    'rng:mf_init': ('host', 'ure_host_mf_init or Tensor.normal_ fill every element'),
    'rng:draw_seed': ('host', 'Tensor.random_ fills the one element'),
    'rng:epoch_seeds': ('host', 'Tensor.random_ fills every element'),
    'rng:_HostPool.take': ('host', 'ure_host_randperm / ure_host_randperm_tags write every element the taker asked for'),
    'rng:epoch_perms': ('host', 'ure_host_randperm writes every row'),
    'rng:epoch_tags': ('host', 'ure_host_randperm_tags writes every row'),
    'rng:epoch_perms_async': ('routine', 'Q3'), 'rng:_DrawsTask.make_buffers': ('routine', 'Q3'), 'rng:make_buffers_together': ('routine', 'Q3'),
    'rng:_shuffle_scratch': ('job', _REQUEST), 'rng:device_tags': ('job', _REQUEST),
    # ---- method/
    'method.sisa:exchange_tables': ('collective', 'dist.all_gather_into_tensor writes recv whole (gloo: the host stage whole, then recv.copy_(host))'),
    'method.utils:MF.forward': ('entry', _SCORE),
    'method.utils:_dense_rows': ('routine', 'C1'), 'method.utils:singleKmeans': ('routine', 'C2'),
}


def check_inventory(table=None):
    """What tests/test_cpu_poison_inventory.py asserts: every allocating function has a class, no entry is stale, every note points
    at something that exists."""
    table = INVENTORY if table is None else table
    found, spans = allocating_functions()
    missing = sorted(n for n in found if n not in table)
    assert not missing, f'no memory class for {missing}: they draw uninitialised memory; run them in a case of tests/test_gpu_routine_memory.py (or name the class) in INVENTORY'
    stale = sorted(n for n in table if n not in found)
    assert not stale, f'{stale} no longer draw uninitialised memory: take them out of INVENTORY'
    root = os.path.dirname(HERE)
    for name, (klass, note) in table.items():
        assert klass in CLASSES, (name, klass)
        if klass == 'routine':
            assert note and all(c in CASES for c in note.split()), f'{name}: {note!r} names no case of this module'
        elif klass in ('job', 'entry'):
            path, test = note.split('::')
            assert os.path.exists(os.path.join(root, path)), note
            with open(os.path.join(root, path)) as fh:
                assert f'def {test}(' in fh.read(), f'{name}: {note} does not exist'
            if klass == 'job':
                assert path in ('tests/test_gpu_job_memory.py', 'tests/test_gpu_nmf.py'), note
        elif klass == 'meta':
            module, qual = name.split(':')
            defs = [s for s in spans[os.path.realpath(os.path.join(PKG, *module.split('.')) + '.py')] if s[2] == name]
            lines = found[name]
            assert module == 'ops' and defs and all(any(first <= ln <= last and fake for first, last, _, fake in defs) for ln in lines), name
        else:
            assert note, f'{name}: name the call that overwrites the buffer'


def credited(case_name):
    return {n for n, (klass, note) in INVENTORY.items() if klass == 'routine' and case_name in note.split()}


# ================================================================== helpers of the cases
def _np(a):
    if torch.is_tensor(a):
        return a.detach().contiguous().cpu().numpy().copy()
    if isinstance(a, (bytes, str)):
        return np.frombuffer(a if isinstance(a, bytes) else a.encode(), np.uint8).copy()
    return np.array(a)


def _pack(out):
    torch.cuda.synchronize()
    return {name: _np(a) for name, a in out.items()}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


class Case:
    """run(tmp) -> {name: array}; check_reference(got) holds the 0x00 run to the family's own bar."""
    name = ''

    def inputs(self):
        pass


# ---------------------------------------------------------------- B1, B2: GcnJob(loss='bpr')
class BprJobCase(Case):
    """audit: the job draws no uninitialised memory at all -- GcnJob.__init__ takes its pool, tags, err, row_loss, the loss series and the
    BPR buffers (neg, map_n, usr_n, off_n, w, the index scratch) from torch.zeros.  neg is written whole by ure_bpr_sample and off_n /
    map_n / usr_n whole by ure_bpr_index at every epoch's first step, before the step's coef pass and walks read them; ure_bpr_index's
    scratch is covered by its guard-zone case.  So a stale offset cannot be read; the run shows that the four fills (which reach the
    job only through what the graph and the uploads draw) change nothing, and that the index of the LAST epoch is the contract's."""

    def __init__(self, name, case):
        self.name, self.case = name, case

    def run(self, tmp):
        c = self.case
        assert c.no_u > 0 and c.no_i > 0 and np.bincount(c.iid).max() > 64 and c.N % c.B != 0 and c.epochs >= 2
        job = c.job()
        job.run()
        out = dict(zip(('padded U', 'padded V', 'padded P', 'padded Q', 'M'), (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])))
        out.update(zip(('U', 'V', 'P', 'Q'), (*job.tables(0), *job.base_tables())))
        out.update({name: job._bpr[name] for name in ('neg', 'off_n', 'map_n', 'usr_n', 'w')})
        out.update(err=job._err, tag=job._tag, row_loss=job._row_loss, loss=job.epoch_loss(0))
        out = _pack(out)
        job.close()
        return out

    def check_reference(self, got):
        from ultrare_amd import bpr
        c = self.case
        ref = bpr_cases.reference(c)
        run = dict(U=[got['U']], V=[got['V']], P=[got['P']], Q=[got['Q']], loss=got['loss'] / c.N)
        E_k = bpr_cases.distance(ref['f64'], run)
        print(f'{self.name}: E_k {E_k:.3g} E_y {ref["E_y"]:.3g} bound {ref["bound"]:.3g}')
        assert ref['E_y'] > 0 and E_k <= ref['bound'], (E_k, ref['E_y'], ref['bound'])
        neg = ref['f64']['neg'][-1]
        assert _same(got['neg'], neg)
        g = c.host()[0]
        for name, want in zip(('off_n', 'map_n', 'usr_n'), bpr.neg_index_ref(neg, g.row_u, c.n_item)):
            assert _same(got[name], want), name


# ---------------------------------------------------------------- A1, A2: GcnJob(attr=...)
class AttrJobCase(Case):
    """The case test_skipped_steps_are_counted_and_leave_the_step_plain builds, with a second epoch in its own random order: every user
    of group 2 sits in one batch of the first epoch, so four of its five steps are skipped, and none of the second.
    audit: masks, rows, counts, grad, valid, out, both scratches and the per-epoch dis / skipped come from torch.zeros in
    _attr_buffers.  masks is written whole by ure_attr_step_masks at step 0 of every epoch; rows (-1 behind the selected ones) and
    counts whole by ure_attr_select at every step before the loss entry and ure_attr_add_grad read them; dis[e] and skipped[e] are
    accumulators that start from those zeros, one slot per epoch, and are only ever added to.  grad and out keep the last valid
    step's values through a skipped step, where valid = 0 keeps ure_attr_add_grad from reading them."""

    def __init__(self, name, var):
        self.name, self.var, self.case = name, var, None

    def inputs(self):
        if self.case is None:
            c = attr_train_cases.Case(40, 24, 8, 600, 128, 2, 1, seed=91, var=self.var, no_i=2)
            c.id2 = np.array([9, 11])
            rest, mine = np.flatnonzero(~np.isin(c.uid, c.id2)), np.flatnonzero(np.isin(c.uid, c.id2))
            assert 0 < len(mine) <= c.B
            c.orders = np.stack([np.concatenate([mine, rest]).astype(c.orders.dtype), c.orders[1]])
            self.case = c

    def run(self, tmp):
        c = self.case
        job = c.job()
        job.run()
        out = dict(zip(('padded U', 'padded V', 'padded P', 'padded Q', 'M'), (*job.padded_tables(0), *job.base_tables(padded=True), job._t['M'])))
        out.update(zip(('U', 'V', 'P', 'Q'), (*job.tables(0), *job.base_tables())))
        out.update(loss=job.epoch_loss(0), dis=job.epoch_dis(), skipped=job.epoch_skipped())
        out.update({'attr ' + name: job._attr[name] for name in ('masks', 'rows', 'counts', 'grad', 'valid', 'out')})
        out = _pack(out)
        job.close()
        return out

    def check_reference(self, got):
        c = self.case
        both = attr_train_cases.reference(c)
        ref = both['f64']
        skipped = got['skipped']
        assert 0 < int(skipped.sum()) < c.steps * c.epochs and skipped[0] == c.steps - 1, skipped       # added to, and left alone
        assert skipped.tolist() == ref['skipped'].tolist()
        base = got['loss'] + c.eta * got['dis']
        run = dict(U=[got['U']], V=[got['V']], P=[got['P']], Q=[got['Q']], loss=np.sqrt(base / c.N) if c.loss == 'mse' else base / c.N)
        E_k = attr_train_cases.distance(ref, run)
        print(f'{self.name}: E_k {E_k:.3g} E_y {both["E_y"]:.3g} bound {both["bound"]:.3g} dis {got["dis"]} ref {ref["dis"]}')
        assert E_k <= both['bound'], (E_k, both['bound'])
        assert np.abs(got['dis'] / ref['dis'] - 1.0).max() <= 1e-5


# ---------------------------------------------------------------- K1: the attacker
class AttackCase(Case):
    """audit: attack_fit draws stats, params, loss and scores, _ProbeRun the training scratch.  stats is written whole by
    ure_attack_standardize before ure_attack_train reads it, params (p_out) and loss [folds, epochs] whole by ure_attack_train, scores
    by ure_attack_score under the fold plan, which covers every position; all three entries and the scratch are guard-zone cases.
    auc_counts / confusion_counts / attack_scores are one entry each on outputs they own.  fold_of is an upload."""
    name = 'K1'
    SETTINGS = {'mlp': dict(attack_cases.SETTINGS, epochs=2), 'logit': dict(attack_cases.LOGISTIC, epochs=2)}    # one Adam step per epoch

    def inputs(self):
        if not hasattr(self, 'X'):
            self.X, self.id1, self.id2 = attack_cases.table(True)
            assert (len(self.id1) + len(self.id2)) % 64 != 0

    def run(self, tmp):
        from ultrare_amd import engine
        out = {}
        n1, n2 = len(self.id1), len(self.id2)
        pos, neg = np.arange(n1), np.arange(n1, n1 + n2)
        for tag, s in self.SETTINGS.items():
            Xt = _dev(self.X)
            groups = engine.GroupRows(self.id1, self.id2, len(self.X), Xt.device)
            fit = engine.attack_fit(Xt, groups, s['hidden'], s['folds'], s['epochs'], s['lr'], s['l2'], s['seed'])
            counts, flag = engine.auc_counts(fit.scores, pos, neg)
            confusion = engine.confusion_counts(fit.scores, pos, neg, 0.5)
            other = engine.attack_scores(fit, Xt, groups.host[::-1].copy(), fold=1)
            out.update({f'{tag} {name}': a for name, a in dict(
                X=Xt, params=fit.params, stats=fit.stats, fold_of=fit.fold_of, scores=fit.scores, loss=fit.loss, auc=counts, nan_flag=flag,
                confusion=confusion, transfer=other).items()})
        return _pack(out)

    def check_reference(self, got):
        from ultrare_amd import attack as A
        for tag, s in self.SETTINGS.items():
            r64, rows, n1, n2, fold_of, p0 = attack_cases.fit_contract(self.X, self.id1, self.id2, s, np.float64)
            r32 = attack_cases.fit_contract(self.X, self.id1, self.id2, s, np.float32)[0]
            scores = got[f'{tag} scores']
            assert _same(got[f'{tag} X'], self.X) and np.array_equal(got[f'{tag} fold_of'], fold_of)
            e_k, e_y = np.abs(scores - r64['scores']).max(), np.abs(r32['scores'] - r64['scores']).max()
            print(f'{self.name} {tag}: E_k {e_k:.3g} E_y {e_y:.3g}')
            assert e_k <= 4 * max(e_y, ULP32)
            assert np.array_equal(got[f'{tag} stats'].view(np.int32), r32['stats'].view(np.int32))
            assert _rel(got[f'{tag} params'], r64['params']) <= 4 * max(_rel(r32['params'], r64['params']), ULP32)
            loss = got[f'{tag} loss']
            assert loss.shape == r64['loss'].shape == (s['folds'], s['epochs']) and np.abs(loss - r64['loss']).max() <= 1e-5 * r64['loss'].max()
            pos, neg = np.arange(n1), np.arange(n1, n1 + n2)
            assert int(got[f'{tag} nan_flag'][0]) == 0 and tuple(got[f'{tag} auc'].tolist()) == A.auc_counts_ref(scores, pos, neg)
            assert tuple(got[f'{tag} confusion'].tolist()) == A.confusion_ref(scores, pos, neg, 0.5)
            want = A.score_ref(self.X, rows[::-1], None, got[f'{tag} params'][1:2], got[f'{tag} stats'][1:2], s['hidden'])
            assert np.abs(got[f'{tag} transfer'] - want).max() <= 4 * ULP32


# ---------------------------------------------------------------- V1: the adversarial loop
class AdversarialCase(Case):
    """audit: one _ProbeRun scratch, one stats, grad, p and auc_ws serve every round, beside four [rounds, ...] logs.  Round t runs
    ure_attack_standardize (writes stats whole) -> ure_attack_train (reads params in place: round 0's are the clone of the uploaded p0;
    writes loss[t] whole) -> ure_adv_input_grad (writes grad and p whole, every position being in exactly one fold group of perm / off,
    which are uploads made on the host from fold_host) -> ure_auc_counts (writes counts[t] and flags[t]; its scratch is a guard-zone
    case) -> the elementwise update, and reg[t] is assigned.  Every row of every log is written by its own round; nothing of round
    t - 1 but params and X, which are meant to carry over, is read by round t."""
    name = 'V1'

    def inputs(self):
        if not hasattr(self, 'X'):
            self.X, self.id1, self.id2 = attack_cases.table(True)
            assert adv_cases.SHORT['rounds'] >= 3

    def run(self, tmp, plant=False):
        from ultrare_amd import engine
        s, out = adv_cases.SHORT, {}
        for tag, stream in (('cur', None), ('side', torch.cuda.Stream())):
            Xt = _dev(self.X)
            groups = engine.GroupRows(self.id1, self.id2, len(self.X), Xt.device)
            fit = engine.adversarial_unlearn(Xt, groups, s['hidden'], s['folds'], s['rounds'], s['disc_epochs'], s['disc_lr'], s['l2'], s['lr'], s['eta'],
                                             s['alpha'], (0.5, 0.5), s['seed'], stream=stream)
            torch.cuda.synchronize()
            out.update({f'{tag} {name}': a for name, a in dict(
                X=Xt, params=fit.params, stats=fit.stats, scores=fit.scores, loss=fit.loss, counts=fit.counts, nan_flags=fit.nan_flags, reg=fit.reg,
                grad=fit.grad, fold_of=fit.fold_of).items()})
        if plant:
            out['planted'] = torch.empty(7, device='cuda')
        return _pack(out)

    def check_reference(self, got):
        """The assertions of tests/test_gpu_adv.py::test_three_rounds_within_the_float32_yardstick."""
        from ultrare_amd import attack as A
        s, X = adv_cases.SHORT, self.X
        m64, log64, rows, n1, n2, fold_of, p0, _ = adv_cases.play(X, self.id1, self.id2, np.float64, **s)
        m32, log32 = adv_cases.play(X, self.id1, self.id2, np.float32, **s)[:2]
        for name in ('X', 'params', 'counts', 'stats', 'scores', 'loss', 'nan_flags', 'reg', 'grad'):
            assert _same(got['cur ' + name], got['side ' + name]), name
        moved = got['cur X']
        assert np.array_equal(got['cur fold_of'], fold_of)
        other = np.setdiff1d(np.arange(len(X)), rows)
        assert np.array_equal(moved[other], X[other])
        for name, dev, a32, a64 in (('rows', moved[rows], m32[rows], m64[rows].astype(np.float64)), ('params', got['cur params'], log32['params'], log64['params']),
                                    ('grad', got['cur grad'], log32['grad'], log64['grad']), ('stats', got['cur stats'], log32['stats'], log64['stats'])):
            e_k, e_y = _rel(dev, a64), _rel(a32, a64)
            print(f'{self.name} {name}: E_k {e_k:.3g} E_y {e_y:.3g}')
            assert e_k <= 4 * max(e_y, ULP32), name
        p_dev = got['cur scores']
        assert np.abs(p_dev - log64['p']).max() <= 4 * max(np.abs(log32['p'] - log64['p']).max(), ULP32)
        counts = got['cur counts']
        assert not got['cur nan_flags'].any()
        assert tuple(counts[-1]) == A.auc_counts_ref(p_dev, np.arange(n1), np.arange(n1, n1 + n2))
        for t in range(s['rounds']):
            p64 = log64['p_rounds'][t]
            b = 4 * max(np.abs(log32['p_rounds'][t] - p64).max(), ULP32)
            close = int((np.abs(p64[:n1, None] - p64[None, n1:]) < 2 * b).sum())
            gt64, eq64 = int((p64[:n1, None] > p64[None, n1:]).sum()), int((p64[:n1, None] == p64[None, n1:]).sum())
            assert abs(int(counts[t, 0]) - gt64) <= close and abs(int(counts[t, 0] + counts[t, 1]) - (gt64 + eq64)) <= close
        loss = got['cur loss']
        assert loss.shape == (s['rounds'], s['folds'], s['disc_epochs'])
        assert np.abs(loss[:, :, 0] - log64['loss_first']).max() <= 1e-5 * log64['loss_first'].max()
        assert np.abs(loss[:, :, -1] - log64['loss_last']).max() <= 1e-5 * log64['loss_last'].max()
        assert np.allclose(got['cur reg'], log64['reg'], rtol=1e-5)


# ---------------------------------------------------------------- N1: the influence solve and the Newton update
class InfluenceCase(Case):
    """audit: inf_solve draws Ap, t and the dot scratch and reuses them every iteration; x, state, log_rr and log_flag are torch.zeros, r
    and p copies of b.  An iteration writes t whole (ure_inf_coef, every CSR entry) before both walks read it, the walks write Ap whole
    (every row, +0.0 on an inactive one: the walk entry's guard-zone cases) before dot(p, Ap) and ure_inf_cg_xr read it, and
    ure_inf_dot's scratch is written before its second level reads it (its own case).  inf_matvec draws e, t, HU and HV per call, in that order of writing and reading.  log_rr / log_flag behind the last iteration
    are zeros and are cut off (rr = log_rr[:ran]).  newton_unlearn calls inf_coef, inf_grad, inf_objective and inf_solve afresh every
    step: nothing of step 1 but the tables reaches step 2."""
    name = 'N1'
    # (tag, case, curvature, damping, iters): converged, damped full Hessian, out of iterations (stops at `iters`), and case C
    SOLVES = (('a gn', 'a', 'gn', 0.0, 512), ('a full', 'a', 'full', 3.0, 512), ('a short', 'a', 'gn', 0.0, 5), ('c gn', 'c', 'gn', 0.0, 512))

    def inputs(self):
        if not hasattr(self, 'cases'):
            from ultrare_amd import influence
            a, c = influence_cases.case_a(), influence_cases.case_c()
            c_active = influence.active_rows(c.g)[:2]
            assert not c_active[0][c.deleted].any() and not a.active[0][5]                    # emptied rows, a frozen row
            self.cases = {'a': (a, a.active), 'c': (c, c_active)}
            self.rhs = {k: influence.grad_ref(x.g, x.U, x.V, x.r, x.l2, act) for k, (x, act) in self.cases.items()}

    def run(self, tmp):
        from ultrare_amd import engine
        from ultrare_amd.method import utils
        out = {}
        for tag, which, curvature, damping, iters in self.SOLVES:
            (c, active), (gU, gV) = self.cases[which], self.rhs[which]
            g = engine.GcnGraph(c.uid, c.iid, c.rating, c.n_user, c.n_item)
            xU, xV, log = engine.inf_solve(g, _dev(c.U), _dev(c.V), _dev(-gU), _dev(-gV), c.l2, damping, curvature, active, None, iters, 1e-8)
            out.update({f'{tag} xU': xU, f'{tag} xV': xV, f'{tag} rr': log['rr'], f'{tag} flag': log['flag'],
                        f'{tag} end': [log['iters_run'], log['status']]})
        for which, (c, active) in self.cases.items():                       # the matrix-vector product on its own, as a caller of the solve's pieces makes it
            P, Q = influence_cases.direction(c, 3)
            g = engine.GcnGraph(c.uid, c.iid, c.rating, c.n_user, c.n_item)
            HU, HV = engine.inf_matvec(g, _dev(c.U), _dev(c.V), _dev(P), _dev(Q), c.l2, 0.05, 'full', active)
            out.update({f'{which} matvec U': HU, f'{which} matvec V': HV})
        c = self.cases['c'][0]
        model = utils.MF.from_tables(_dev(c.U), _dev(c.V))
        logs = utils.newton_unlearn(model, (c.uid, c.iid, c.rating), l2=c.l2, steps=2)
        out.update({'newton U': model.user_mat.weight, 'newton V': model.item_mat.weight, 'newton steps': len(logs)})
        for i, log in enumerate(logs):
            out.update({f'newton {i} rr': log['rr'], f'newton {i} F': [log['F_before'], log['F_after']],
                        f'newton {i} end': [int(log['applied']), log['iters_run'], log['status']]})
        return _pack(out)

    def check_reference(self, got):
        from ultrare_amd import influence
        for tag, which, curvature, damping, iters in self.SOLVES:
            (c, active), (gU, gV) = self.cases[which], self.rhs[which]
            wU, wV, wlog = influence.solve_ref(c.g, c.U, c.V, c.r, -gU, -gV, c.l2, damping, curvature, active, None, iters, 1e-8)
            assert got[f'{tag} end'].tolist() == [wlog['iters_run'], wlog['status']], tag
            assert wlog['iters_run'] >= 3 and (wlog['iters_run'] == iters and wlog['status'] == 0) == (tag == 'a short'), (tag, wlog['iters_run'], wlog['status'])
            assert got[f'{tag} rr'].tobytes() == wlog['rr'].tobytes() and got[f'{tag} flag'].tobytes() == wlog['flag'].tobytes(), tag
            assert _same(got[f'{tag} xU'], wU) and _same(got[f'{tag} xV'], wV), tag
        for which, (c, active) in self.cases.items():
            P, Q = influence_cases.direction(c, 3)
            wU, wV = influence.matvec_ref(c.g, c.U, c.V, c.r, P, Q, c.l2, 0.05, 'full', active)
            assert _same(got[f'{which} matvec U'], wU) and _same(got[f'{which} matvec V'], wV), which
        c = self.cases['c'][0]
        wU, wV, wlogs = influence_cases.case_c_steps(2)
        assert _same(got['newton U'], wU) and _same(got['newton V'], wV)
        assert not got['newton U'][c.deleted].any()
        assert int(got['newton steps']) == len(wlogs) == 2
        for i, w in enumerate(wlogs):
            assert got[f'newton {i} end'].tolist() == [int(w['applied']), w['iters_run'], w['status']] and w['applied'], i
            assert got[f'newton {i} rr'].tobytes() == w['rr'].tobytes() and got[f'newton {i} F'].tolist() == [w['F_before'], w['F_after']], i


# ---------------------------------------------------------------- R1: ALS sweeps and fold-in
class RidgeCase(Case):
    """The synthetic set of tests/test_gpu_ridge.py: 2,000 x 500, 50,000 ratings, k = 16, user 7 and item 3 without one (empty
    segments).  audit: ridge_rows draws X and the two status words per call; ure_ridge_rows writes every row of X (the zero row for
    an empty segment, NaN for a failed one) and both status words (its guard-zone case).  als_sweeps hands the X of one half sweep
    to the next as the fixed table: a row nobody wrote would be read there."""
    name = 'R1'
    L2, L2_N, K = 0.5, 0.02, 16

    def inputs(self):
        if not hasattr(self, 'uid'):
            from test_gpu_ridge import normal_table
            n_user, n_item, n = 2000, 500, 50000
            rs = np.random.RandomState(11)
            uid, iid = rs.randint(0, n_user, n), rs.randint(0, n_item, n)
            uid[uid == 7] = 8
            iid[iid == 3] = 4
            self.uid, self.iid, self.r = uid, iid, (rs.randint(1, 6, n) / 5.0).astype(np.float32)
            self.U0, self.V0 = normal_table(n_user, self.K, 12), normal_table(n_item, self.K, 13)
            self.pick = np.isin(uid, rs.permutation(n_user)[:40])
            self.n_user = n_user

    def run(self, tmp):
        from ultrare_amd.method.utils import MF, als_sweeps, fold_in
        triple = (self.uid, self.iid, self.r)
        model = MF.from_tables(_dev(self.U0), _dev(self.V0))
        one, obj1 = als_sweeps(model, triple, self.L2, self.L2_N, sweeps=1)
        two, obj2 = als_sweeps(model, triple, self.L2, self.L2_N, sweeps=2)
        part = tuple(a[self.pick] for a in triple)
        users, rows = fold_in([model], part, self.L2, self.L2_N, item_table=0)
        users_m, rows_m = fold_in([model, one], part, self.L2, self.L2_N, item_table='mean')
        return _pack({'U1': one.user_mat.weight, 'V1': one.item_mat.weight, 'obj1': obj1, 'U2': two.user_mat.weight, 'V2': two.item_mat.weight,
                      'obj2': obj2, 'fold users': users, 'fold rows': rows, 'fold mean users': users_m, 'fold mean rows': rows_m,
                      'U0': model.user_mat.weight, 'V0': model.item_mat.weight})

    def check_reference(self, got):
        from test_gpu_ridge import check_against_contract
        from ultrare_amd import ridge
        uid, iid, r, U0, V0, k, l2, l2_n = self.uid, self.iid, self.r, self.U0, self.V0, self.K, self.L2, self.L2_N
        assert _same(got['U0'], U0) and _same(got['V0'], V0)
        U1, V1, obj = got['U1'], got['V1'], got['obj1']
        want = [ridge.ridge_objective(a, b, uid, iid, r, l2, l2_n) for a, b in ((U0, V0), (U1, V0), (U1, V1))]
        assert obj.shape == (3,) and all(abs(a - b) <= 1e-12 * b for a, b in zip(obj, want)), (obj, want)
        assert not U1[7].any() and not V1[3].any()
        off, idx, val, _ = ridge.segment_csr(uid, iid, r, self.n_user)
        check_against_contract(U1, V0, k, off, idx, val, l2, l2_n, what='R1 first half')
        obj2 = got['obj2']
        assert obj2.shape == (5,) and obj2[:3].tobytes() == obj.tobytes()
        assert all(b <= a * (1 + 1e-8) for a, b in zip(obj2[:-1], obj2[1:]))
        assert abs(obj2[-1] - ridge.ridge_objective(got['U2'], got['V2'], uid, iid, r, l2, l2_n)) <= 1e-12 * obj2[-1]
        pu, pi, pr = uid[self.pick], iid[self.pick], r[self.pick]
        users = np.unique(pu)
        perm = np.argsort(pu, kind='stable')
        poff = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(users, pu), minlength=len(users)))])
        mean = ((V0.astype(np.float64) + V1.astype(np.float64)) / 2).astype(np.float32)
        for name, V in (('fold', V0), ('fold mean', mean)):
            assert np.array_equal(got[name + ' users'], users) and got[name + ' rows'].shape == (len(users), k)
            check_against_contract(got[name + ' rows'], V, k, poff, pi[perm], pr[perm], l2, l2_n, what='R1 ' + name)


# ---------------------------------------------------------------- R2: WMF sweeps and fold-in
class WmfCase(Case):
    """_synthetic() of tests/test_gpu_wmf.py: 300 x 200, 6,000 observations, k = 8, user 7 and item 3 without one.
    audit: gram draws G0 and its scratch, wridge_rows X and two status words, per call.  ure_gram writes the whole packed triangle from
    chunk sums it wrote first, ure_wridge_rows every row of X and both status words (guard-zone cases).  WmfSweeps keeps GU / GV beside
    U / V and replaces both after every half: the Gram matrix a half reads is always the one of the table it reads."""
    name = 'R2'
    ALPHA, L2 = 40.0, 0.1

    def inputs(self):
        if not hasattr(self, 'uid'):
            self.uid, self.iid, self.r = wmf_cases.rating_set(300, 200, 6000, seed=11, skip_user=7, skip_item=3)
            self.U0, self.V0 = wmf_cases.normal_table(300, 8, 12), wmf_cases.normal_table(200, 8, 13)
            self.pick = np.isin(self.uid, [4, 5, 250, 299])

    def run(self, tmp):
        from ultrare_amd.method.utils import MF, wmf_fold_in, wmf_sweeps
        triple, out = (self.uid, self.iid, self.r), {}
        model = MF.from_tables(_dev(self.U0), _dev(self.V0))
        for l2_n in (0.0, 0.02):
            one, obj1 = wmf_sweeps(model, triple, self.ALPHA, self.L2, l2_n, sweeps=1)
            two, obj2 = wmf_sweeps(model, triple, self.ALPHA, self.L2, l2_n, sweeps=2)
            out.update({f'{l2_n} U1': one.user_mat.weight, f'{l2_n} V1': one.item_mat.weight, f'{l2_n} obj1': obj1,
                        f'{l2_n} U2': two.user_mat.weight, f'{l2_n} V2': two.item_mat.weight, f'{l2_n} obj2': obj2})
        part = tuple(a[self.pick] for a in triple)
        users, rows = wmf_fold_in([model], part, self.ALPHA, self.L2, 0.02, item_table=0)
        users_m, rows_m = wmf_fold_in([model, model], part, self.ALPHA, self.L2, 0.02)
        out.update({'fold users': users, 'fold rows': rows, 'fold mean users': users_m, 'fold mean rows': rows_m})
        return _pack(out)

    def check_reference(self, got):
        from ultrare_amd import ridge
        from ultrare_amd import wmf as W
        uid, iid, r, U0, V0, k = self.uid, self.iid, self.r, self.U0, self.V0, 8
        off, idx, val, _ = ridge.segment_csr(uid, iid, r, 300)
        wg, wb = W.confidence_ref(val, self.ALPHA)
        for l2_n in (0.0, 0.02):
            U1, V1, obj = got[f'{l2_n} U1'], got[f'{l2_n} V1'], got[f'{l2_n} obj1']
            _, _, want = W.wmf_sweeps_ref(U0, V0, uid, iid, r, self.ALPHA, self.L2, l2_n, sweeps=1)
            assert obj.shape == (3,) and all(abs(a - b) <= 1e-12 * b for a, b in zip(obj, want)), (obj, want)
            assert obj[2] <= obj[1] <= obj[0] and not U1[7].any() and not V1[3].any()
            wmf_cases.check_rows(U1, V0, k, off, idx, wg, wb, W.gram_ref(V0, k), self.L2, l2_n, what=f'R2 first half, l2_n={l2_n}')
            obj2 = got[f'{l2_n} obj2']
            assert obj2.shape == (5,) and obj2[:3].tobytes() == obj.tobytes()
            assert all(b <= a * (1 + 1e-6) for a, b in zip(obj2[:-1], obj2[1:]))
            assert not got[f'{l2_n} U2'][7].any() and not got[f'{l2_n} V2'][3].any()
        assert got['fold users'].tolist() == [4, 5, 250, 299] == got['fold mean users'].tolist()
        assert _same(got['fold rows'], got['0.02 U1'][[4, 5, 250, 299]]) and _same(got['fold mean rows'], got['fold rows'])


# ---------------------------------------------------------------- C1 .. C5: the grouping routines
def _toy_embedding():
    return np.load(os.path.join(G, 'ot_toy.npz'))['X']


def _cluster_gold():
    import hashlib
    gold = np.load(os.path.join(G, 'cluster_toy.npz'))
    X64 = gold['X'].astype(np.float64)
    D = np.empty((len(X64), len(X64)), dtype=np.float32)                   # (toy_D of tests/test_gpu_cluster.py)
    for i in range(0, len(X64), 128):
        D[i:i + 128] = np.sqrt(((X64[i:i + 128, None, :] - X64[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    assert hashlib.sha256(D.tobytes()).hexdigest() == str(gold['D_sha256'])
    return gold, D


def _ratings():
    """The fixture `ratings` of tests/test_gpu_sparse_pair.py: 200 users x 400 items, wider than group.DENSE_MAX_ITEMS."""
    from scipy import sparse
    rs = np.random.RandomState(77)
    mat = sparse.random(200, 400, density=0.06, random_state=rs, format='csr', dtype=np.float32)
    mat.data[:] = rs.randint(1, 11, mat.nnz) / 2.0
    return mat, np.ascontiguousarray(mat.toarray(), dtype=np.float32)


class OtClusterCase(Case):
    """ot_cluster, three rounds: the exact LP and Sinkhorn on CSR rows (crafted('columns') of tests/test_gpu_sparse_group.py: an empty
    column, a column that holds every user) and on dense rows (tests/golden/ot_toy.npz).
    audit: _dense_rows draws dist_d, cent_d and counts_d once and reuses them every round: ure_ot_cost writes dist_d whole before the
    solver reads it, ure_ot_centroids_members writes cent_d and counts_d whole (a cluster without a member: its NaN row) before
    cent_d comes to the host.  _csr_rows draws nothing itself: csr_cost and csr_centroids allocate per call and their entries write
    every byte (Ct's padding columns come from torch.zeros).  ot_sinkhorn draws label, v, cost_min and its scratch per call.
    ure_ot_potentials keeps its state in an allocation of its own (the list of what the helper cannot reach).
    The dense exact route is held to the numpy clusterer of the oracle, oracle.cpu_ref.ot_cluster (the reference's loop with an exact
    LP), under the same seed and the same three rounds: equal labels, equal float64 inertia, the bar of
    tests/test_gpu_surface.py::test_ot_cluster_bit_exact."""
    name, K, ROUNDS = 'C1', 4, 3

    def inputs(self):
        if not hasattr(self, 'halves'):
            from test_gpu_sparse_group import crafted
            from ultrare_amd import sparse_group as sg
            self.halves, self.X = crafted('columns'), _toy_embedding()
            np.random.seed(0)
            first = sg.dense_rows(self.halves[0], np.random.choice(self.halves[0].shape[0], size=self.K, replace=False))
            self.reg_csr = float(np.median(sg.csr_cost_ref(self.halves[0], first)))

    def run(self, tmp):
        from ultrare_amd.method.utils import ot_cluster
        out = {}
        for tag, X, kw in (('csr exact', self.halves, {}), ('csr sinkhorn', self.halves, dict(solver='sinkhorn', reg=self.reg_csr)),
                           ('dense exact', self.X, {}), ('dense sinkhorn', self.X, dict(solver='sinkhorn'))):
            np.random.seed(0)
            inertia, label = ot_cluster(X, self.K, max_iters=self.ROUNDS, **kw)
            out.update({tag + ' inertia': np.float64(inertia), tag + ' label': label})
            if 'sinkhorn' in tag:
                out[tag + ' stats'] = np.asarray(ot_cluster.sinkhorn_stats, dtype=np.float64)
        return _pack(out)

    def check_reference(self, got):
        from oracle import cpu_ref as O
        from test_cpu_sinkhorn import ot_cluster_contract
        from test_gpu_sparse_group import replay, warm_exact_solver
        from ultrare_amd import engine
        n = self.halves[0].shape[0]
        np.random.seed(0)
        want_inertia, want_label = replay(self.halves, self.K, warm_exact_solver(n, self.K), max_iters=self.ROUNDS)
        assert np.array_equal(got['csr exact label'], want_label) and float(got['csr exact inertia']) == float(want_inertia)

        def solve(dist):
            return engine.ot_sinkhorn(torch.from_numpy(dist).cuda(), self.reg_csr, 1000, 1e-9, want_u=False)['label'].cpu().numpy()
        np.random.seed(0)
        want_inertia, want_label = replay(self.halves, self.K, solve, max_iters=self.ROUNDS)
        assert np.array_equal(got['csr sinkhorn label'], want_label) and float(got['csr sinkhorn inertia']) == float(want_inertia)
        assert len(got['csr sinkhorn stats']) >= 2 and len(got['dense sinkhorn stats']) >= 2                # >= 2 rounds: the buffers were reused
        np.random.seed(0)
        want_inertia, want_label, rounds, want_stats = ot_cluster_contract(self.X, self.K, max_iters=self.ROUNDS)
        stats = got['dense sinkhorn stats']
        assert len(stats) == rounds and [int(s[0]) for s in stats] == [s[0] for s in want_stats]
        assert np.array_equal(got['dense sinkhorn label'], want_label) and float(got['dense sinkhorn inertia']) == float(want_inertia)
        np.random.seed(0)
        want_inertia, want_label = O.ot_cluster(self.X, self.K, max_iters=self.ROUNDS)
        assert np.array_equal(got['dense exact label'], want_label) and np.float64(got['dense exact inertia']) == np.float64(want_inertia)


class KmeansCase(Case):
    """kmeans(balanced=True), n_init = 2, max_iter = 3, on crafted() of tests/test_gpu_sparse_kmeans.py (203 x 97, rows 0 and 202 empty,
    row 2 full) as sparse rows and as the dense array, and one plain singleKmeans run of each.  The reference of the 0x00 run is the
    numpy clusterer of the oracle under the same seed -- oracle.cpu_ref.kmeans / single_kmeans, equal labels and equal inertia, the bar of
    tests/test_gpu_surface.py::test_kmeans_kernels_vs_oracle_random -- for the dense route, and the CSR route must give the dense
    route's bytes (test_single_kmeans_on_the_csr_equals_the_dense_route).
    audit: singleKmeans draws dist_d, label_d and counts_d once per run: ure_kmeans_cost writes dist_d whole before it comes to the
    host, label_d is copied whole from the host's labels before ure_kmeans_centroids reads it (a stale int32 label there would index
    cent_d at will -- it is never read before that copy), counts_d is written whole by the entry.  _single_kmeans_csr draws
    nothing itself; csr_kmeans_cost, balanced_fill and csr_kmeans_centroids allocate per call, and balanced_fill's scratch is sized
    and written by its own entry (guard-zone case)."""
    name, K = 'C2', 5

    def inputs(self):
        if not hasattr(self, 'halves'):
            from test_gpu_sparse_kmeans import crafted
            from ultrare_amd import sparse_group as sg
            self.halves = crafted()
            self.dense = sg.dense_rows(self.halves[0], np.arange(self.halves[0].shape[0])).astype(np.float32)

    def _runs(self):
        from ultrare_amd.method import utils
        out, n = {}, self.halves[0].shape[0]
        for tag, src in (('csr', self.halves), ('dense', self.dense)):
            np.random.seed(3)
            out[tag + ' label'] = utils.kmeans(self.K, n, src, balanced=True, n_init=2, max_iter=3)
            np.random.seed(4)
            label, inertia = utils.singleKmeans(self.K, n, src, False, 3)
            out.update({tag + ' plain label': label, tag + ' plain inertia': np.float64(inertia)})
        return out

    def run(self, tmp):
        return _pack(self._runs())

    def check_reference(self, got):
        from oracle import cpu_ref as O
        n = self.halves[0].shape[0]
        np.random.seed(3)
        want = O.kmeans(self.K, self.dense, True, 2, 3)
        np.random.seed(4)
        want_plain, want_inertia = O.single_kmeans(self.K, self.dense, False, 3)
        assert np.array_equal(got['dense label'], want) and np.array_equal(got['dense plain label'], want_plain)
        assert float(got['dense plain inertia']) == want_inertia
        for name in ('label', 'plain label', 'plain inertia'):
            assert _same(got['csr ' + name], got['dense ' + name]), name
        assert np.bincount(got['csr label'], minlength=self.K).max() <= int(np.ceil(n / self.K))


class PairSources(Case):
    """What C3, C4 and C5 share: the given array and the embedding of tests/golden/cluster_toy.npz, and sparse rows beside their dense form."""

    def inputs(self):
        if not hasattr(self, 'D'):
            self.gold, self.D = _cluster_gold()
            self.mat, self.X = _ratings()

    def _sparse(self, fn, metric):
        """fn on the sparse rows and on the dense array, under one seed -> the two label vectors."""
        out = []
        for src in (self.mat, self.X):
            np.random.seed(1234)
            out.append(fn(4, 200, src, balanced=True, n_init=2, max_iter=6, metric=metric))
        return out


class KmedoidsCase(PairSources):
    """kmedoids on the given array of tests/golden/cluster_toy.npz under the golden's own settings (seed 11, n_init = 3, max_iter = 10:
    the reference exists for these, and they keep >= 2 inits and >= 2 rounds) and, streamed from sparse rows, n_init = 2 and
    max_iter = 6 as tests/test_gpu_sparse_pair.py runs it against the dense route.
    audit: pair_rowsum, pair_cols draw their output per call and their entries write it whole (guard-zone cases of
    tests/test_gpu_abi_memory.py and tests/test_gpu_sparse_pair.py); nothing is kept between rounds but the host's medoid list."""
    name = 'C3'

    def run(self, tmp):
        from ultrare_amd.method import utils
        out, n = {}, len(self.D)
        for balanced in (False, True):
            np.random.seed(11)
            label, inertia, medoids = utils.singleKmedoids(4, n, self.D, balanced, 10, return_medoids=True)
            np.random.seed(11)
            out.update({f'given {balanced} single label': label, f'given {balanced} inertia': np.float32(inertia), f'given {balanced} medoids': medoids,
                        f'given {balanced} label': utils.kmedoids(4, n, self.D, balanced=balanced, n_init=3, max_iter=10)})
        out['csr label'], out['dense label'] = self._sparse(utils.kmedoids, 'euclidean')
        return _pack(out)

    def check_reference(self, got):
        for balanced in (False, True):
            tag = f'km_k4_{"bal" if balanced else "plain"}'
            np.testing.assert_array_equal(got[f'given {balanced} single label'], self.gold[tag + '_labels'][0])
            assert got[f'given {balanced} inertia'] == self.gold[tag + '_inertia'][0]
            np.testing.assert_array_equal(got[f'given {balanced} medoids'], self.gold[tag + '_medoids'][0])
            np.testing.assert_array_equal(got[f'given {balanced} label'], self.gold[tag + '_label'])
        assert _same(got['csr label'], got['dense label']) and np.bincount(got['csr label'], minlength=4).max() <= 50


class LpaCase(PairSources):
    """singleLPA on the given array against the golden under its margins (tests/test_gpu_cluster.py::test_lpa_given_matches_reference),
    lpa(n_init = 2) streamed from sparse rows against the dense route.  lpa on the given array with n_init = 2, max_iter = 3 has no
    reference at that input: it is collected for the comparison between fills, and held to the balanced group size.
    audit: pair_label_expsum draws W per call; the entry writes every (user, group) cell, a group without a member as 0."""
    name = 'C4'

    def run(self, tmp):
        from ultrare_amd.method import utils
        out, n = {}, len(self.D)
        for balanced in (False, True):
            np.random.seed(13)
            label, inertia = utils.singleLPA(4, n, self.D, balanced, 10, max_iter=10)
            out.update({f'given {balanced} single label': label, f'given {balanced} inertia': np.float64(inertia)})
        np.random.seed(13)
        out['given label'] = utils.lpa(4, n, self.D, balanced=True, n_init=2, max_iter=3)
        out['csr label'], out['dense label'] = self._sparse(utils.lpa, 'manhattan')
        return _pack(out)

    def check_reference(self, got):
        for balanced in (False, True):
            tag = f'lpa_{"bal" if balanced else "plain"}'
            want, margin = self.gold[tag + '_labels'][0], self.gold[tag + '_margin'][0]
            differ = np.flatnonzero(got[f'given {balanced} single label'] != want)
            assert np.all(margin[differ] < 1e-5), (differ[:10], margin[differ][:10])
            inertia = float(got[f'given {balanced} inertia'])
            assert abs(inertia - self.gold[tag + '_inertia'][0]) <= 1e-6 * abs(self.gold[tag + '_inertia'][0])
        assert np.bincount(got['given label'], minlength=4).max() <= int(np.ceil(len(self.D) / 4))
        assert _same(got['csr label'], got['dense label']) and np.bincount(got['csr label'], minlength=4).max() <= 50


class NeighborCase(PairSources):
    """findNeighbor (cache dir = the test's tmp_path) on the embedding of tests/golden/cluster_toy.npz and on sparse rows.
    audit: pair_knn draws dist, idx and the split scratch per call; the entry writes every (query, neighbour) cell, the scratch's
    partial lists before its merge reads them (guard-zone cases, with and without splits)."""
    name = 'C5'

    def run(self, tmp):
        from ultrare_amd import engine
        from ultrare_amd.method import utils
        X = self.gold['X']
        out = {'emb dist': engine.pair_knn(X, 10, 'euclidean')[0]}
        for tag, src, n in (('emb', X, len(X)), ('csr', self.mat, 200), ('dense', self.X, 200)):
            idx, val = utils.findNeighbor(f'{tmp}/{tag}_', src, n, var='euclidean', n_neighbor=10)
            with open(f'{tmp}/{tag}_euclidean.npy', 'rb') as f:
                out.update({tag + ' idx': idx, tag + ' val': val, tag + ' file': f.read()})
        return _pack(out)

    def check_reference(self, got):
        from test_gpu_cluster import _d64
        X, idx, val, dist = self.gold['X'], got['emb idx'], got['emb val'], got['emb dist']
        g_idx, g_val = self.gold['nn_euclidean_idx'], self.gold['nn_euclidean_val']
        assert _same(val, (-dist).astype(np.float16))
        for u in range(len(X)):
            ref = _d64(X, [u], 'euclidean')[0]
            np.testing.assert_allclose(dist[u], ref[idx[u]], rtol=1e-5, atol=1e-5)
            assert np.all(np.diff(dist[u]) >= 0)
            for p in np.flatnonzero(idx[u] != g_idx[u]):
                a, b = ref[idx[u, p]], ref[g_idx[u, p]]
                assert abs(a - b) <= 1e-5 * max(abs(a), abs(b), 1e-6), (u, p, a, b)
        spacing = np.spacing(np.abs(g_val).astype(np.float16)).astype(np.float32)
        assert np.all(np.abs(val.astype(np.float32) - g_val.astype(np.float32)) <= spacing + 1e-6)
        assert _same(got['csr idx'], got['dense idx']) and _same(got['csr val'], got['dense val']) and _same(got['csr file'], got['dense file'])


# ---------------------------------------------------------------- S1: the combiner, recommendation, ranking
class ServeCase(Case):
    """Three MF tables of 90 users x 1,100 items at d = 8 (two item splits in recommend: rec_splits of csrc/rec_select.h wants 512 items a
    split, so 600 would be one and the partial lists in the scratch would not exist), three groups of 30 users; user 5 has trained on
    every item (an excluded user: nothing is left to recommend).  The loaders are made anew in every run: a loader keeps its EvalSet, whose buffers must come out of
    the run's own fill.
    audit: combine_stats draws its scratch and the stats vector per Newton pass (ure_combine_stats writes the vector whole from
    partials it wrote first); recommend draws scores, items and the split scratch per call, rank_pairs the ranks and its scratch
    (guard-zone cases with two item splits).  EvalSet draws top_rating, which ure_eval_rank_ratings writes whole in __init__ before
    any ranking reads it as an index; pred, hits, ndcg and sse are torch.zeros and serve baseTest calls with three and then two
    models: ure_score / ure_score_weighted write pred[:n] and every sse partial at each call (first = 1), ure_eval_users every user."""
    name = 'S1'
    N_USER, N_ITEM, D = 90, 1100, 8

    def inputs(self):
        if not hasattr(self, 'tables'):
            rs = np.random.RandomState(91)
            self.groups = [list(range(30 * g, 30 * (g + 1))) for g in range(3)]
            self.train = [np.stack([rs.randint(30 * g, 30 * (g + 1), 400), rs.randint(0, self.N_ITEM, 400), rs.randint(1, 6, 400) / 5.0]) for g in range(3)]
            self.test = [np.stack([rs.randint(30 * g, 30 * (g + 1), 100), rs.randint(0, self.N_ITEM, 100), rs.randint(1, 6, 100) / 5.0]) for g in range(3)]
            scale = 0.5 * self.D ** -0.25
            self.tables = [((rs.standard_normal((self.N_USER, self.D)) * scale + 0.3).astype(np.float32),
                            (rs.standard_normal((self.N_ITEM, self.D)) * scale + 0.3).astype(np.float32)) for _ in range(3)]
            import scipy.sparse as sp
            u = np.concatenate([a[0] for a in self.train] + [np.full(self.N_ITEM, 5)]).astype(np.int64)
            i = np.concatenate([a[1] for a in self.train] + [np.arange(self.N_ITEM)]).astype(np.int64)
            self.excl = sp.csr_matrix((np.ones(len(u), np.float32), (u, i)), shape=(self.N_USER, self.N_ITEM))
            self.users = np.arange(self.N_USER)

    def _loaders(self):
        from ultrare_amd.read import RatingData, loadData
        return ([loadData(RatingData(a), 200, 0) for a in self.train], loadData(RatingData(np.hstack(self.test)), 200, 0, False))

    def _models(self):
        from ultrare_amd.method.utils import MF
        return [MF.from_tables(_dev(U), _dev(V)) for U, V in self.tables]

    def run(self, tmp):
        from ultrare_amd import _native as nv
        from ultrare_amd.method import utils
        models, (trd, tot), out = self._models(), self._loaders(), {}
        assert nv.lib().ure_recommend_scratch(self.N_USER, self.N_ITEM, 10) > 0                          # more than one item split
        for link in ('linear', 'logistic'):
            c = utils.fit_combiner(models, trd, link, l2=1e-3, groups=self.groups)
            out.update({f'{link} W': c.W, f'{link} loss': np.asarray(c.loss_after, dtype=np.float64), f'{link} iters': np.asarray(c.iters)})
            s, i = utils.recommend(models, self.users, 10, self.excl, combiner=c)
            m = utils.rank_eval(models, tot, self.excl, combiner=c)
            out.update({f'{link} rec scores': s, f'{link} rec items': i, f'{link} rank': [m[k] for k in sorted(m)],
                        f'{link} base': utils.baseTest(tot, models, combiner=c)})
        s, i = utils.recommend(models, self.users, 10, self.excl)
        m = utils.rank_eval(models, tot, self.excl)
        out.update({'rec scores': s, 'rec items': i, 'rank': [m[k] for k in sorted(m)], 'base 3': utils.baseTest(tot, models),
                    'pred 3': tot.eval_set().predictions()})
        out.update({'base 2': utils.baseTest(tot, models[:2]), 'pred 2': tot.eval_set().predictions()})        # the same EvalSet, fewer models
        s, i = utils.recommend(models[:2], self.users[::-1].copy(), 7)
        out.update({'rec2 scores': s, 'rec2 items': i})
        return _pack(out)

    def check_reference(self, got):
        import test_gpu_combine_rank as CR
        import test_gpu_rank as RK
        import test_gpu_recommend as RC
        from oracle import cpu_ref as O
        from ultrare_amd import engine
        from ultrare_amd.method import utils
        models, (trd, tot) = self._models(), self._loaders()
        tabs = [utils.padded_tables(m)[:2] for m in models]
        d = utils.padded_tables(models[0])[2]
        ex = engine.exclusion_rows(self.excl, self.users)
        P = RC.oracle_scores(tabs, d, self.users)
        ws, wi = RC.oracle_topk(P, 10, ex)
        assert (wi[5] == -1).all() and (wi[6] >= 0).all()                                                   # the excluded user
        RC.assert_same((torch.from_numpy(got['rec scores']), torch.from_numpy(got['rec items'])), (ws, wi))
        rev = self.users[::-1].copy()
        RC.assert_same((torch.from_numpy(got['rec2 scores']), torch.from_numpy(got['rec2 items'])), RC.oracle_topk(RC.oracle_scores(tabs[:2], d, rev), 7))
        q_users, off, items = utils.relevant_pairs(tot, self.N_ITEM)
        qex = engine.exclusion_rows(self.excl, q_users)
        want = RK._numpy_metrics(off, RK.oracle_ranks(RC.oracle_scores(tabs, d, q_users), (off, items), qex), (10, 20))
        RK._assert_metrics(dict(zip(sorted(want), got['rank'].tolist())), {k: float(v) for k, v in want.items()})
        uid, iid, r = tot.dataset.triples()
        for link in ('linear', 'logistic'):
            c = utils.fit_combiner(models, trd, link, l2=1e-3, groups=self.groups)                          # (outside the poison)
            assert c.W.shape == (3, 4) and c.W.tobytes() == got[f'{link} W'].tobytes()
            W, gou = c.on_device(tabs[0][0].device, self.N_USER)
            sc = CR.yardstick(tabs, d, self.users, self.N_ITEM, (c.link_code, W, gou))
            CR.same_topk((torch.from_numpy(got[f'{link} rec scores']), torch.from_numpy(got[f'{link} rec items'])), CR.oracle_topk(sc, 10, ex))
            want = utils.rank_metrics(off, CR.ranks_of(sc[q_users], (off, items), qex))
            assert dict(zip(sorted(want), got[f'{link} rank'].tolist())) == {k: float(v) for k, v in want.items()}
        for name, n_models in (('3', 3), ('2', 2)):
            # baseTest from the device's predictions, at the bar of tests/test_gpu_combine.py; the predictions are the mean's, bit for bit
            pred, base = got['pred ' + name], got['base ' + name]
            want = O.eval_from_pred(uid.astype(np.int64), r, pred, 200)
            assert abs(base[0] - want[0]) <= 1e-6 * want[0] and abs(base[1] - want[1]) <= 1e-12 and abs(base[2] - want[2]) <= 1e-12
            every = RC.oracle_scores(tabs[:n_models], d, np.arange(self.N_USER))
            assert _same(pred, every[uid, iid]), name


# ---------------------------------------------------------------- S2: NeuMF serving
class NmfServeCase(Case):
    """Two models of nmf_cases.stage_model at the smallest STAGE_SHAPES entry, 40 users x 600 items.
    audit: nmf_recommend / nmf_rank_pairs draw their outputs and one scratch per call, written by their entries before the merge reads
    them (tests/test_gpu_nmf_rank.py::test_raw_abi_in_guard_zones)."""
    name = 'S2'
    N_USER, N_ITEM = 40, 600

    def inputs(self):
        if not hasattr(self, 'models'):
            (self.k, self.layers), rs = nmf_cases.STAGE_SHAPES[0], np.random.RandomState(5)
            self.models = [nmf_cases.stage_model(self.k, self.layers, self.N_USER, self.N_ITEM, seed) for seed in (1, 2)]
            self.users = rs.permutation(self.N_USER)[:33]
            self.test = np.stack([rs.randint(0, self.N_USER, 300), rs.randint(0, self.N_ITEM, 300), rs.randint(1, 6, 300) / 5.0])
            import scipy.sparse as sp
            u, i = rs.randint(0, self.N_USER, 900), rs.randint(0, self.N_ITEM, 900)
            self.excl = sp.csr_matrix((np.ones(900, np.float32), (u, i)), shape=(self.N_USER, self.N_ITEM))

    def _models(self):
        from ultrare_amd.method.utils import NMF
        return [NMF.from_tables(*(_dev(np.ascontiguousarray(t, dtype=np.float32)) for t in m), self.k, self.layers) for m in self.models]

    def _loader(self):
        from ultrare_amd.read import RatingData, loadData
        return loadData(RatingData(self.test), 200, 0, False)

    def run(self, tmp):
        from ultrare_amd.method import utils
        models, tot = self._models(), self._loader()
        s, i = utils.recommend_nmf(models, self.users, 10, self.excl)
        s1, i1 = utils.recommend_nmf(models[:1], self.users, 10)
        m = utils.rank_eval_nmf(models, tot, self.excl)
        return _pack({'rec scores': s, 'rec items': i, 'rec1 scores': s1, 'rec1 items': i1, 'rank': [m[k] for k in sorted(m)]})

    def check_reference(self, got):
        import test_gpu_nmf_rank as NR
        from ultrare_amd import engine, nmf
        from ultrare_amd.method import utils
        dev = NR.on_device(self.models)
        sc = NR.device_scores(dev, self.k, self.layers, self.users, self.N_ITEM)
        ex = engine.exclusion_rows(self.excl, self.users)
        NR.same_topk((torch.from_numpy(got['rec scores']), torch.from_numpy(got['rec items'])), NR.oracle_topk(sc, 10, ex))
        sc1 = NR.device_scores(dev[:1], self.k, self.layers, self.users, self.N_ITEM)
        NR.same_topk((torch.from_numpy(got['rec1 scores']), torch.from_numpy(got['rec1 items'])), NR.oracle_topk(sc1, 10, None))
        q_users, off, items = utils.relevant_pairs(self._loader(), self.N_ITEM)
        qex = engine.exclusion_rows(self.excl, q_users)
        ranks = nmf.rank_ref(None, self.k, self.layers, q_users, (off, items), qex, scores=NR.device_scores(dev, self.k, self.layers, q_users, self.N_ITEM),
                             n_item=self.N_ITEM)
        want = utils.rank_metrics(off, ranks)
        assert dict(zip(sorted(want), got['rank'].tolist())) == {k: float(v) for k, v in want.items()}


# ---------------------------------------------------------------- U1: attribute unlearning after training
class AttrUnlearnCase(Case):
    """The first case of tests/golden/attr_toy.npz, the table of tests/test_gpu_attr.py's loop tests, three steps, in place: the whole
    user table and the item table are collected.
    audit: per step mmd_bandwidth draws bw and a scratch, mmd_loss_grad sums, grad and a scratch, u2u_loss_grad value, grad and a
    scratch; each is written whole by its entry before the elementwise update reads it (guard-zone cases), and the last step's
    want_grad = False passes no grad at all.  Nothing is kept from step to step but the table."""
    name = 'U1'

    def inputs(self):
        if not hasattr(self, 'X'):
            g = np.load(os.path.join(G, 'attr_toy.npz'))                   # (the fixture `gold` of tests/test_gpu_attr.py)
            self.g, self.X = g, np.load(os.path.join(G, 'kmeans_toy.npz'))['X'].astype(np.float32)
            n1, n2, d = (int(v) for v in g['cases'][0])
            self.n1, self.n2, self.d = n1, n2, d
            self.id1, self.id2 = np.arange(n1), np.arange(n1, n1 + n2)
            self.kw = dict(eta=float(g['loop_eta']), alpha=float(g['loop_alpha']), lr=float(g['loop_lr']), steps=int(g['loop_steps']))
            assert self.kw['steps'] == 3

    def _model(self, X):
        import test_gpu_attr as TA
        return TA._toy_model(X, self.d)

    def run(self, tmp):
        from ultrare_amd.method import utils
        out = {}
        for var, kw in (('d2d', self.kw), ('u2u', dict(self.kw, lr=3e-4))):
            model = self._model(self.X)
            log = utils.attribute_unlearn(model, self.id1, self.id2, var, **kw)
            out.update({f'{var} U': model.user_mat.weight, f'{var} V': model.item_mat.weight,
                        f'{var} log': np.asarray([log['dis'], log['reg'], log['bandwidth']], dtype=np.float64)})
        return _pack(out)

    def check_reference(self, got):
        from ultrare_amd import attr_unlearn as au
        X, d, m = self.X[:, :self.d], self.d, self.n1 + self.n2
        want, _ = au.attribute_unlearn_ref(X, self.id1, self.id2, 'd2d', **self.kw)
        dist_device = np.abs(got['d2d U'].astype(np.float64)[:m] - want[:m]).max()
        dist_reference = np.abs(self.g['loop_rows'].astype(np.float64) - want[:m]).max()
        print(f'{self.name}: device vs contract {dist_device:.3g}, reference float32 vs contract {dist_reference:.3g}')
        assert dist_device <= 4 * dist_reference
        # u2u: no family test holds the moved rows to a bound at any input (attr_unlearn.py derives one for the value and the gradient of
        # one call, not for a loop); the loop's dis log is held to the contract's as tests/test_gpu_attr.py::
        # test_fine_tune_touches_only_the_groups_and_is_reproducible holds it for both variants (its rtol, 1e-4), the rows to the fills
        want_log = au.attribute_unlearn_ref(X, self.id1, self.id2, 'u2u', **dict(self.kw, lr=3e-4))[1]
        assert np.allclose(got['u2u log'][0], want_log['dis'], rtol=1e-4)
        for var in ('d2d', 'u2u'):
            assert np.array_equal(got[f'{var} U'][m:], X[m:]) and not np.array_equal(got[f'{var} U'][:m], X[:m])
            assert _same(got[f'{var} V'], self._model(self.X).item_mat.weight.cpu().numpy())
            assert got[f'{var} log'].shape == (3, 4) and got[f'{var} log'][1, 0] == 0.0


# ---------------------------------------------------------------- Q1, Q2: one request each
class RequestCase(Case):
    """Sisa learn on three shards of the toy set, two epochs, then unlearn of five users of shard 1: the model bytes and the logs, as
    tests/test_gpu_nmf.py::test_sisa_request_on_poisoned_memory collects them.  The reference of the 0x00 run is what the family's
    own request test asserts of the same calls: finite logs, shard 1 alone retrained, the other shards' bytes unchanged.
    audit (Q1): the request adds to B1 the EvalSet series of every shard (lane buffers drawn once per lane and reused from epoch to
    epoch: each series call writes base, pred, sse, hits and ndcg for its members before ure_eval_reduce reads them) and the merge.
    audit (Q2): Scratch's 'wmf' backbone drives WmfSweeps (R2) and evaluates after every sweep."""

    def __init__(self, name, backbone):
        self.name, self.backbone = name, backbone

    def run(self, tmp):
        import copy
        from ultrare_amd.method.sisa import Sisa
        T = __import__('test_gpu_bpr' if self.backbone == 'lightgcn' else 'test_gpu_wmf')
        idx, trd, ted, tot = T._loaders(3)
        s = Sisa(T.Param(2), self.backbone, 3, idx)
        torch.manual_seed(42)
        ml = list(s.learn(trd, ted, tot, 0, ''))
        out = self._models('learn', ml)
        del_user = [int(u) for u in idx[1][:5]]
        idx2, trd2, ted2, tot2 = T._loaders(3, del_user) if self.backbone == 'lightgcn' else T._loaders(3, del_user, idx)
        s2 = Sisa(T.Param(2), self.backbone, 3, idx2)
        torch.manual_seed(42)
        ml2 = list(s2.unlearn([copy.deepcopy(m) for m in ml], trd2, ted2, tot2, del_user, 0, ''))
        out.update(self._models('unlearn', ml2))
        out['retrained'] = list(s2.retrained)
        for tag, sisa in (('learn', s), ('unlearn', s2)):
            out[tag + ' log0'] = repr(sorted((k, v) for k, v in sisa.log0.items() if k != 'time'))
            out[tag + ' log'] = repr(sorted((k, [float(x) for x in np.ravel(v)]) for k, v in sisa.log.items() if k != 'time'))
            out[tag + ' finite'] = bool(all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for k, v in sisa.log.items() if k != 'time'))
        return _pack(out)

    @staticmethod
    def _models(tag, ml):
        out = {}
        for i, m in enumerate(ml):
            out[f'{tag} U{i}'], out[f'{tag} V{i}'] = m.user_mat.weight, m.item_mat.weight
            for j, t in enumerate(getattr(m, 'base', None) or ()):
                out[f'{tag} base{i}.{j}'] = t
        return out

    def check_reference(self, got):
        assert got['retrained'].tolist() == [1] and bool(got['learn finite']) and bool(got['unlearn finite'])
        assert _same(got['learn V0'], got['unlearn V0']) and _same(got['learn V2'], got['unlearn V2']) and not _same(got['learn V1'], got['unlearn V1'])
        assert all(np.isfinite(a).all() for name, a in got.items() if a.dtype.kind == 'f')


# ---------------------------------------------------------------- L1: the stateless step calls beside the graph jobs
class StepCallsCase(Case):
    """gcn_step_tags, gcn_propagate, gcn_loss_grad, bpr_negatives, bpr_neg_index and bpr_loss_grad as a caller outside a job makes them,
    every step of GRAD_CASE of tests/test_gpu_lightgcn.py / tests/test_gpu_bpr.py (37 x 29, 300 triples, B = 128: the last step holds 44
    and leaves rows without an entry) at d = 8.  Unlike the jobs (B1 .. A2), these draw everything from torch.empty, and two of them are
    compositions: gcn_loss_grad (residual, two walks, the loss fold) and bpr_loss_grad (the index, the coefficient pass, two walks, the
    fold).  The references are the family's own: lightgcn.loss_grad_ref / propagate_ref and bpr.sample_ref / neg_index_ref / coef_ref /
    walks_ref bit for bit (w to one ulp, the losses to 1e-12), as test_loss_gradient_equals_the_contract_bit_for_bit and
    test_coefficients_and_walks_equal_the_contract hold them.
    audit: err, pred, Gu, Gi, row_loss and loss of gcn_loss_grad: ure_gcn_residual writes err and pred whole (+0.0 outside the batch)
    before the walks read err, each walk writes every row of its G (+0.0 for a row without an entry) and the user walk every row_loss
    entry before ure_gcn_step_loss folds them into loss with first = 1.  bpr_loss_grad: off_n / map_n / usr_n are written whole by
    ure_bpr_index before ure_bpr_grad_item reads them as offsets and indices (a stale one would be a wild read: it cannot be, the index
    call precedes the walks on the same stream); w, x, sp, sn whole by ure_bpr_coef; the rest as above."""
    name, D = 'L1', 8

    def inputs(self):
        if not hasattr(self, 'case'):
            from test_cpu_score_contract import tables as mixed_tables
            self.case = c = bpr_cases.Case(37, 29, 4, 300, 128, 1, 2, seed=77, no_u=5, no_i=4)
            (U, V), = mixed_tables(700 + self.D, self.D, 1, n_user=c.n_user, n_item=c.n_item)
            self.U, self.V = (U * np.float32(0.25)).astype(np.float32), (V * np.float32(0.25)).astype(np.float32)

    def run(self, tmp):
        from ultrare_amd import engine as E
        c, out = self.case, {}
        g = c.graph()
        Ud, Vd = _dev(self.U), _dev(self.V)
        tag = E.gcn_step_tags(g, c.orders[0], c.B)
        neg = E.bpr_negatives(g, c.key, 0)
        out.update(zip(('tag', 'neg', 'off_n', 'map_n', 'usr_n'), (tag, neg, *E.bpr_neg_index(g, neg))))
        out.update({'prop csr': E.gcn_propagate(g, 'csr', Vd), 'prop csc': E.gcn_propagate(g, 'csc', Ud)})
        for step in range(c.steps):
            out.update(zip((f'mse {step} {n}' for n in ('Gu', 'Gi', 'loss', 'err', 'pred')), E.gcn_loss_grad(g, tag, step, Ud, Vd, want_pred=True)))
            out.update(zip((f'bpr {step} {n}' for n in ('Gu', 'Gi', 'loss', 'w', 'x', 'sp', 'sn')), E.bpr_loss_grad(g, tag, step, Ud, Vd, neg)))
        return _pack(out)

    def check_reference(self, got):
        from ultrare_amd import bpr, lightgcn
        c, U, V = self.case, self.U, self.V
        g, off_d, col_d = c.host()
        neg = bpr.sample_ref(g, off_d, col_d, c.key, 0)
        index = bpr.neg_index_ref(neg, g.row_u, c.n_item)
        assert _same(got['neg'], neg) and all(_same(got[n], w) for n, w in zip(('off_n', 'map_n', 'usr_n'), index))
        for side, X in (('csr', V), ('csc', U)):
            off, idx, s_src, s_dst, _, _ = g.side(side)
            assert _same(got['prop ' + side], lightgcn.propagate_ref(off, idx, s_src, s_dst, X)), side
        for step in range(c.steps):
            batch = c.orders[0][step * c.B:(step + 1) * c.B]
            Gu, Gi, loss, pred = lightgcn.loss_grad_ref(g, U, V, c.rating, batch)
            in_csr = ~np.isnan(pred[g.pos])
            assert in_csr.sum() == len(batch) and np.array_equal(got['tag'] == step, in_csr)
            assert _same(got[f'mse {step} Gu'], Gu) and _same(got[f'mse {step} Gi'], Gi), step
            assert got[f'mse {step} pred'][in_csr].tobytes() == pred[g.pos][in_csr].tobytes()
            assert not got[f'mse {step} pred'][~in_csr].any() and not got[f'mse {step} err'][~in_csr].any()
            assert abs(float(got[f'mse {step} loss'][0]) - loss) <= 1e-12 * abs(loss)
            w_ref, x_ref, sp_ref, sn_ref = bpr.coef_ref(g, U, V, neg, in_csr)
            w, x = got[f'bpr {step} w'], got[f'bpr {step} x']
            assert _same(x, x_ref) and _same(got[f'bpr {step} sp'], sp_ref) and _same(got[f'bpr {step} sn'], sn_ref), step
            w64 = -1.0 / (1.0 + np.exp(x[in_csr].astype(np.float64)))
            ulp = np.spacing(np.abs(w64).astype(np.float32)).astype(np.float64)
            assert (np.abs(w[in_csr].astype(np.float64) - w64) <= ulp).all() and (w[in_csr] <= 0).all()
            assert w[~in_csr].tobytes() == bytes(4 * int((~in_csr).sum())) == x[~in_csr].tobytes()
            want_u, want_i, row_loss = bpr.walks_ref(g, index, U, V, neg, w, x, in_csr)
            assert _same(got[f'bpr {step} Gu'], want_u) and _same(got[f'bpr {step} Gi'], want_i), step
            want_loss = lightgcn.fold_256(row_loss)
            assert abs(float(got[f'bpr {step} loss'][0]) - want_loss) <= 1e-12 * want_loss
        assert len(batch) == 44


class HostTagsRequestCase(Case):
    """Q3: the MF request of tests/test_gpu_surface.py (three shards, two epochs, learn and two unlearn calls, held to the goldens of the
    real reference inside check_sisa_against_reference itself) with URE_DEVICE_TAGS=0, side by side and one shard after the other: the
    epochs' batch tags are then expanded by the host's threads and arrive on the device in chunks, a path the requests of
    tests/test_gpu_job_memory.py (device tags) never take.
    audit: the device copy of the tags is drawn whole from torch.empty (epoch_perms_async: one piece; _DrawsTask.make_buffers and
    make_buffers_together: one block, a view per shard) and filled by on_dev[c0:c1].copy_(host[c0:c1]) chunk by chunk on a side
    stream; TrainJob.run launches an epoch only behind the arrival of the chunk that holds it, so no step reads tags that were not
    copied yet.  The pinned host rows come from rng._HostPool and are written whole by ure_host_randperm_tags before their copy.
    epoch_perms_async serves a request only when a table is too small for the generator's skip-ahead (fewer than 16 elements), which
    no golden has: it is run as Scratch's prepare_shard(defer=True) calls it, its device tags handed to a TrainJob of one toy shard
    whose tables and losses are held to the C oracle at the bar of tests/test_gpu_job_memory.py (MfCase.check_reference)."""
    name = 'Q3'

    def inputs(self):
        if not hasattr(self, 'job'):
            import test_gpu_job_memory as J
            from ultrare_amd import rng
            self.job = J.MfCase('Q3 job', B=3000)
            parts, inits, perms = self.job.inputs()
            torch.manual_seed(42)                                        # (MfCase.inputs' own draws again, for the seeds it does not keep)
            rng.mf_init(self.job.n_user, self.job.n_item, self.job.k)
            self.seeds = rng.epoch_seeds(self.job.E, True)
            assert torch.equal(rng.epoch_perms(self.seeds, len(parts[0][0])), perms[0])

    def _direct(self):
        from ultrare_amd import engine, rng
        parts, inits, _ = self.job.inputs()
        n, B = len(parts[0][0]), self.job.B
        tags = rng.epoch_perms_async(self.seeds, n, threads=2, pooled=True, device=engine._device(), tags_batch=rng.tags_batch_for(n, B)).result()
        assert tags.is_cuda and tags.dtype == torch.int16 and rng.Arrival.of(tags).whole
        job = engine.TrainJob([engine.ShardData(*parts[0], self.job.n_user, self.job.n_item)], inits, [tags], self.job.k, B, self.job.E, 1e-3, 0.1, 0.9, 0.95)
        job.run()
        U, V = job.tables(0)
        out = _pack({'U0': U, 'V0': V, 'sse0': job.epoch_sse(0), 'tags': tags})
        job.close()
        return out

    def run(self, tmp):
        from test_gpu_surface import check_sisa_against_reference
        out = {'direct ' + name: a for name, a in self._direct().items()}
        with pytest.MonkeyPatch.context() as m:
            m.setenv('URE_DEVICE_TAGS', '0')
            for tag, parallel in (('side by side', True), ('in turn', False)):
                d = tmp / tag.replace(' ', '_')
                d.mkdir()
                out.update({f'{tag} {name}': b for name, b in check_sisa_against_reference(3, 2, parallel, d).items()})
        return _pack(out)

    def check_reference(self, got):
        assert len(got) > 20                                             # (the goldens were asserted inside the run, under every fill)
        self.job.check_reference({name[len('direct '):]: a for name, a in got.items() if name.startswith('direct ')})


CASES = {c.name: c for c in (
    BprJobCase('B1', bpr_cases.WHOLE_STEP_CASES[0]), BprJobCase('B2', bpr_cases.WHOLE_STEP_CASES[5]),
    AttrJobCase('A1', 'd2d'), AttrJobCase('A2', 'u2u'),
    AttackCase(), AdversarialCase(), InfluenceCase(), RidgeCase(), WmfCase(),
    OtClusterCase(), KmeansCase(), KmedoidsCase(), LpaCase(), NeighborCase(),
    ServeCase(), NmfServeCase(), AttrUnlearnCase(),
    RequestCase('Q1', 'lightgcn'), RequestCase('Q2', 'wmf'), HostTagsRequestCase(), StepCallsCase(),
)}
assert bpr_cases.WHOLE_STEP_CASES[5].layers == 0

_RUNS = {}           # (case name, fill) -> the arrays of that run
_REACHED = {}        # case name -> the inventory functions that allocated in its 0x00 run
_SPANS = []


def run_case(case, fill, monkeypatch, tmp_path, **kw):
    key = (case.name, fill) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        case.inputs()                                    # (host inputs: made once, outside the poison)
        if not _SPANS:
            _SPANS.append(allocating_functions()[1])
        tmp = tmp_path / f'run{len(_RUNS)}'
        tmp.mkdir()
        seen = set()
        t0 = time.perf_counter()
        with poison.active(monkeypatch, fill):
            with monkeypatch.context() as m:
                if fill is not None:
                    watch(m, seen, _SPANS[0])
                _RUNS[key] = case.run(tmp, **kw)
        print(f'{case.name} {FILL_IDS[FILLS.index(fill)]}: run {time.perf_counter() - t0:.2f} s')
        if fill == 0x00 and not kw:
            _REACHED[case.name] = seen
    return _RUNS[key]


@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
@pytest.mark.parametrize('name', list(CASES))
def test_a_routine_gives_the_same_bytes_on_memory_of_every_fill(name, fill, monkeypatch, tmp_path):
    case = CASES[name]
    got = run_case(case, fill, monkeypatch, tmp_path)
    if fill == 0x00:
        assert all(a.size for a in got.values()), [n for n, a in got.items() if not a.size]
        case.check_reference(got)
        missed = credited(name) - _REACHED[name]
        assert not missed, f'{name} is credited in INVENTORY with {sorted(missed)} but its run never allocated there; it reached {sorted(_REACHED[name])}'
        return
    found = differences(run_case(case, 0x00, monkeypatch, tmp_path), got)
    assert not found, f'{name}: fill 0x00 against {FILL_IDS[FILLS.index(fill)]}:\n  ' + '\n  '.join(found)


@pytest.mark.parametrize('fill', [0x5A, 0xFF], ids=['fill0x5a', 'fill0xff'])
def test_a_buffer_nobody_wrote_is_reported_and_nothing_else(fill, monkeypatch, tmp_path):
    """The harness must be able to fail here: V1's run with one more array, torch.empty(7) read back as it came.  differences() names
    exactly that array -- the collection happens inside the poison, and the comparison sees device buffers."""
    case = CASES['V1']
    found = differences(run_case(case, 0x00, monkeypatch, tmp_path, plant=True), run_case(case, fill, monkeypatch, tmp_path, plant=True))
    assert len(found) == 1 and found[0].startswith('planted: 28 byte(s) differ'), found
