"""The host side of tests/test_gpu_routine_memory.py: every function of ultrare_amd/ that draws uninitialised memory (torch.empty,
torch.empty_like, Tensor.new_empty) has a memory class in its INVENTORY -- a case of that module that runs it on poisoned memory, a
job or request test that does, the guard-zone test of the one entry it wraps, a shape-only registration, or host staging that one
call overwrites whole.  A new allocation site without a class fails here, as does a stale entry or a note that points nowhere; and
the scanner and the frame lookup the device run relies on are checked on small sources of their own."""
import sys
import textwrap

import pytest
import torch

import poison
import test_gpu_routine_memory as M


def test_every_allocating_function_is_classified():
    M.check_inventory()
    found, _ = M.allocating_functions()
    assert len(found) == len(M.INVENTORY) >= 82 and len(found['ops:_']) >= 30            # (ops.py's fake registrations share one name)
    assert 'engine:adversarial_unlearn' in found and 'method.utils:_dense_rows' in found and 'ops:_' in found
    assert {klass for klass, _ in M.INVENTORY.values()} == set(M.CLASSES)
    # every case is credited with something or is a job that draws zeros only (its audit says so)
    idle = sorted(name for name in M.CASES if not M.credited(name))
    assert idle == ['A1', 'A2', 'B1', 'B2'], idle


@pytest.mark.parametrize('name', ['engine:adversarial_unlearn', 'method.utils:_dense_rows', 'rng:mf_init'])
def test_removing_a_name_from_the_table_fails(name, monkeypatch):
    table = dict(M.INVENTORY)
    del table[name]
    monkeypatch.setattr(M, 'INVENTORY', table)
    with pytest.raises(AssertionError, match=name.split(':')[1]):
        test_every_allocating_function_is_classified()


def test_a_stale_entry_a_missing_test_and_an_unknown_case_fail():
    with pytest.raises(AssertionError, match='no longer draw'):
        M.check_inventory({**M.INVENTORY, 'engine:unlearn_row_step': ('routine', 'V1')})
    with pytest.raises(AssertionError, match='does not exist'):
        M.check_inventory({**M.INVENTORY, 'engine:gram': ('entry', 'tests/test_gpu_wmf.py::test_nobody_wrote')})
    with pytest.raises(AssertionError, match='names no case'):
        M.check_inventory({**M.INVENTORY, 'engine:gram': ('routine', 'R2 Z9')})
    with pytest.raises(AssertionError, match='ops:mf_score'):
        M.check_inventory({**M.INVENTORY, 'ops:mf_score': ('meta', 'register_fake')})          # not a shape-only registration


SOURCE = '''
import torch

class Job:
    def __init__(self, n):
        self.buf = torch.empty(n)

    def step(self):
        return [torch.zeros(3) for _ in range(2)]


def outer(x):
    def inner():
        return x.new_empty(4)
    pick = (torch.empty if x.numel() else torch.zeros)(2)
    return inner(), pick, (torch.empty_like(x) for _ in range(1)), (lambda: torch.empty(1))


def clean(x):
    return torch.zeros_like(x), x.empty if hasattr(x, 'empty') else None


@some.register_fake
def _(x):
    return x.new_empty(1)
'''


def test_the_scanner_sees_every_form_of_the_call(tmp_path):
    pkg = tmp_path / 'pkg'
    (pkg / 'sub').mkdir(parents=True)
    (pkg / 'a.py').write_text(SOURCE)
    (pkg / 'sub' / 'b.py').write_text('import torch\nBUF = torch.empty(3)\n')
    found, spans = M.allocating_functions(str(pkg))
    assert sorted(found) == ['a:Job.__init__', 'a:_', 'a:outer', 'a:outer.inner', 'sub.b:<module>']
    assert len(found['a:outer']) == 3                     # the conditional callee, the generator expression, the lambda
    defs = spans[str((pkg / 'a.py').resolve())]
    assert [(name, fake) for _, _, name, fake in defs if name == 'a:_'] == [('a:_', True)]
    first = SOURCE.splitlines().index('@some.register_fake') + 1
    assert [s[0] for s in defs if s[2] == 'a:_'] == [first]                                 # a decorated def starts at its decorator
    line = SOURCE.splitlines().index('        return x.new_empty(4)') + 1
    assert M.function_at(spans, str(pkg / 'a.py'), line) == 'a:outer.inner'
    assert M.function_at(spans, str(pkg / 'a.py'), line + 1) == 'a:outer'
    assert M.function_at(spans, str(pkg / 'a.py'), 2) is None and M.function_at(spans, 'elsewhere.py', 5) is None


def test_the_watch_names_the_calling_function_beside_the_poison(tmp_path, monkeypatch):
    """The counting wrapper on top of the poison, on the CPU: the buffers still come back filled, the caller is named by its def -- a
    generator expression and a lambda by the def around them -- and a caller outside the scanned tree is not recorded."""
    pkg = tmp_path / 'pkg2'
    pkg.mkdir()
    (pkg / 'mod.py').write_text(textwrap.dedent('''
        import torch

        def direct(n):
            return torch.empty(n, dtype=torch.uint8)

        def nested(n):
            make = lambda: torch.empty(n, dtype=torch.uint8)
            return list(torch.empty_like(make()) for _ in range(1)) + [make().new_empty(2)]

        def quiet(n):
            return torch.zeros(n)
    '''))
    _, spans = M.allocating_functions(str(pkg))
    monkeypatch.syspath_prepend(str(pkg))
    sys.modules.pop('mod', None)
    import mod
    seen = set()
    with poison.active(monkeypatch, 0x5A):
        with monkeypatch.context() as m:
            M.watch(m, seen, spans)
            a, b = mod.direct(5), mod.nested(3)
            mod.quiet(2)
            torch.empty(3)                                # (this file is outside the tree)
    assert seen == {'mod:direct', 'mod:nested'}
    assert (a == 0x5A).all() and all((t == 0x5A).all() for t in b)
    before = set(seen)
    mod.direct(1)
    assert seen == before and torch.empty is not None      # the wrapper is gone with its context
    sys.modules.pop('mod', None)
