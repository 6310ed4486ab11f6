"""The stencil emitter (``backends/hip_emitter``, ``backends/hip_band``) pinned on the CPU: every row of
``tests/golden/make_emit_golden.py`` — the sources of every plan of the march-plan matrix and of the benchmark shapes,
and direct calls of the emit functions for what no plan reaches — prints the text whose SHA-256
``tests/golden/emit_source_sha.json`` records (generated before any line of the emitter changed). A change that
means to alter a kernel regenerates the JSON; its diff is then the list of kernels that change."""
import importlib.util
import json
import os

import pytest

pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location('make_emit_golden', os.path.join(HERE, 'golden', 'make_emit_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_emitted_sources_match_the_pinned_hashes():
    gen = _generator()
    with open(gen.PATH) as fh:
        want = json.load(fh)
    got = gen.rows()
    assert list(got) == list(want)
    bad = [f'{k}\n    pinned: {want[k]}\n    now:    {got[k]}' for k in want if want[k] != got[k]]
    assert not bad, f'{len(bad)} sources differ:\n' + '\n'.join(bad[:40])
    assert len(want) >= 900 and sum(v.startswith('ERROR') for v in want.values()) < 40
    # the module switch scripts/tune_march.py sets reaches the text
    assert want['emit_pointwise axpy_float32 POINTWISE_NT_LOAD=False'] != want['emit_pointwise axpy_float32']

