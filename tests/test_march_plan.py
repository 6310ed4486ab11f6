"""The march planner (``backends/march_plan.py``, entered through ``hip_kernel.default_march_config`` and
``HipStencilKernel._plan_march``) pinned on the CPU: every row of ``tests/golden/make_march_plan_golden.py`` — kernels ×
shapes × vector widths × tile overrides × environment switches × pointer alignments × launch options — gives the
``MarchConfig`` / launch plan / error recorded in ``tests/golden/march_plan.json`` (generated before the planner was
split into stages). A tuning change regenerates the JSON; its diff is then the list of launches that change."""
import importlib.util
import os

import pytest

pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location('make_march_plan_golden',
                                                  os.path.join(HERE, 'golden', 'make_march_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_march_plans_match_the_pinned_rows():
    gen = _generator()
    with open(gen.PATH) as fh:
        want = gen.decode(fh.read())
    got = gen.rows()
    assert sorted(got) == sorted(want)
    bad = []
    for kname in want:
        keys = list(dict.fromkeys(list(want[kname]) + list(got[kname])))
        bad += [f'{kname} | {k}\n    pinned: {want[kname].get(k)}\n    now:    {got[kname].get(k)}'
                for k in keys if want[kname].get(k) != got[kname].get(k)]
    assert not bad, f'{len(bad)} rows differ:\n' + '\n'.join(bad[:40])
