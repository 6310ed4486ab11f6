"""Sparse and one-sided tap tables (``tests/tap_families.py``) on every stencil schedule.

The schedules print their kernels from the stencil's tap table and branch on it: the band rows assign or accumulate per
plane (``hip_band/rows.py::taps``, the zeroing in ``hip_band/steps.py``, the trimmed steps), the plane ring changes its
depth and feeds "lite" fields from registers (``hip_emitter/geometry.py::lite_fields``, ``march.py``), ``zsum_plan``
groups taps by plane. The workloads drive them with full boxes and symmetric stars; the families here leave planes,
sides, the centre or the x neighbours out.

CPU part: ``oracle.evaluate`` of the derived forward and backward assignments against the plain references (which
states the transpose independently of the autodiff derivation), the C backend against them, what the planners answer
per family (``ELIGIBILITY``), that every launch of the GPU matrix plans onto the schedule its row names (stub
tensors, no device), and a gfx950 compile sweep. GPU part (``-m gpu``): every family, forward and adjoint, on every
row of ``ROWS`` against the plain references, cell by cell (``conftest.assert_cells``); ``shift`` exactly."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

import pystencils_autodiff_amd as pa
from oracle import evaluate as OE
from pystencils_autodiff_amd.backends.hip_band import band_choice, band_plans
from pystencils_autodiff_amd.backends.hip_emitter import MarchConfig, ws_geometry, zsum_plan
from pystencils_autodiff_amd.backends.hip_emitter.geometry import half_ring_ok, lite_fields
from pystencils_autodiff_amd.backends.hip_kernel import HipStencilKernel, default_march_config
from pystencils_autodiff_amd.backends.kernel_ir import StencilKernel
from tests import tap_families as TF
from tests.conftest import assert_cells, assert_close_rel

HERE = os.path.dirname(os.path.abspath(__file__))
F16, F32, F64 = np.float16, np.float32, np.float64
TOL_CPU = {F32: 1e-6, F64: 1e-12}             # tests/test_cpu_backend.py


def _directions(op):
    return (('f', op.forward_assignments), ('b', op.backward_assignments))


def _draw(names, shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.uniform(-1, 1, shape).astype(dtype) for n in names}


def _input_names(name, which):
    return ['u'] if which == 'f' else ['diff' + n for n in TF.outputs(name)]


def _wrap_oracle(ac, arrays, scalars):
    """``oracle.evaluate`` under periodic boundaries: wrap-padded inputs under 'zeros', cropped (the construction of
    ``test_periodic_march.periodic_reference``)."""
    padded = {n: np.pad(np.asarray(a, dtype=np.float64), 1, mode='wrap') for n, a in arrays.items()}
    out = OE.evaluate(ac, padded, scalars, boundary_handling='zeros')
    crop = tuple(slice(1, -1) for _ in next(iter(arrays.values())).shape)
    return {n: a[crop] for n, a in out.items()}


# ------------------------------------------------------------------------------------- CPU: oracle vs plain reference
@pytest.mark.parametrize('bh', ['zeros', 'periodic'])
@pytest.mark.parametrize('name', TF.NAMES_3D + TF.NAMES_2D)
def test_oracle_matches_the_plain_references(name, bh):
    """The derived forward and backward assignments, evaluated by the oracle, are the plain gather and its plain
    transpose: float64 against float64, 1e-14 of the maximum."""
    shape = (5, 6, 7) if TF.ndim(name) == 3 else (6, 7)
    op = pa.AutoDiffOp(TF.collection(name, 'float64'), boundary_handling=bh)
    sc = TF.scalars(name)
    for which, ac in _directions(op):
        ins = _draw(_input_names(name, which), shape, F64, 11)
        got = OE.evaluate(ac, ins, sc, boundary_handling='zeros') if bh == 'zeros' else _wrap_oracle(ac, ins, sc)
        want = TF.reference(name, which, ins, bh, **sc)
        assert set(got) == set(want), (which, sorted(got))
        for n in want:
            assert_close_rel(got[n], want[n], 1e-14, f'{name} {bh} {which} {n}')


@pytest.mark.parametrize('name', TF.NONE_FAMILIES)
def test_interior_only_oracle_is_the_plain_reference_on_the_interior(name):
    """``boundary_handling=None``: the oracle writes the interior box (one ghost layer per axis, whichever axes carry
    taps: ``test_oracle.py``) with the values of the plain reference and leaves the rest zero."""
    shape = (5, 6, 7)
    op = pa.AutoDiffOp(TF.collection(name, 'float64'), boundary_handling=None)
    box = tuple(slice(1, n - 1) for n in shape)
    for which, ac in _directions(op):
        ins = _draw(_input_names(name, which), shape, F64, 12)
        got = OE.evaluate(ac, ins, boundary_handling=None)
        for n, want in TF.reference(name, which, ins, 'zeros').items():
            assert_close_rel(got[n][box], want[box], 1e-14, f'{name} {which} {n}')
            outside = got[n].copy()
            outside[box] = 0
            assert not outside.any()


def test_plain_adjoint_is_the_transpose_of_plain_forward():
    """<A u, d> == <u, Aᵀ d> for the two plain references themselves, under both boundary rules."""
    rng = np.random.default_rng(5)
    u, d = rng.uniform(-1, 1, (4, 5, 6)), rng.uniform(-1, 1, (4, 5, 6))
    for name in TF.FAMILIES:
        taps = TF.numeric(TF.FAMILIES[name], beta=TF.BETAS[0])
        for bh in ('zeros', 'periodic'):
            lhs = float(np.vdot(TF.plain_forward(taps, u, bh), d))
            rhs = float(np.vdot(u, TF.plain_adjoint(taps, d, bh)))
            assert abs(lhs - rhs) <= 1e-13 * len(taps) * u.size, (name, bh, lhs, rhs)


def test_family_tables():
    """The tables are what their names say: tap counts, fixed distinct weights of magnitude 0.1 .. 1 with both signs."""
    counts = {'shift': 1, 'no_zminus': 18, 'only_zplus': 9, 'plane_only': 9, 'x_only': 2, 'no_dx': 9, 'upwind': 4,
              'no_centre': 26, 'q19': 19, 'corners': 8, 'symbol_weight': 4,
              'shift2': 1, 'x_only2': 2, 'y_only2': 2, 'no_centre2': 8, 'corners2': 4}
    assert {n: len(t) for n, t in {**TF.FAMILIES, **TF.FAMILIES_2D}.items()} == counts
    for box in (TF.BOX, TF.BOX2):
        w = list(box.values())
        assert len(set(abs(v) for v in w)) == len(w) and all(0.1 <= abs(v) <= 1 for v in w)
        assert min(w) < 0 < max(w)
    assert (0, 0, 0) not in TF.FAMILIES['no_centre'] and all(o[0] == 1 for o in TF.FAMILIES['only_zplus'])
    assert all(o[2] == 0 for o in TF.FAMILIES['no_dx']) and all(all(o) for o in TF.FAMILIES['corners'])


# ------------------------------------------------------------------------------------------------- CPU: the C backend
def _cpu_kernels(name, dtype, bh):
    """(forward, adjoint) C kernels: every cell written, reads outside the domain zero or wrapped."""
    op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling=bh)
    if bh == 'zeros':
        return op.create_forward_kernel('cpu', ghost_layers=0), op.create_backward_kernel('cpu', ghost_layers=0)
    return op.forward_ast_cpu.compile(), op.backward_ast_cpu.compile()


def _cpu_run(name, dtype, bh, shape, seed):
    """[(which, inputs, {output: array})] of the C kernels."""
    res = []
    for which, k in zip('fb', _cpu_kernels(name, dtype, bh)):
        ins = _draw(_input_names(name, which), shape, dtype, seed)
        outs = {f.name: np.full(shape, np.nan, dtype=dtype) for f in k.ir.fields_written}
        k(**ins, **outs, **TF.scalars(name))
        res.append((which, ins, outs))
    return res


@pytest.mark.parametrize('bh', ['zeros', 'periodic'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', TF.NAMES_3D + TF.NAMES_2D)
def test_c_backend_matches_the_plain_references(name, dtype, bh):
    shape = (5, 6, 7) if TF.ndim(name) == 3 else (6, 7)
    for which, ins, outs in _cpu_run(name, dtype, bh, shape, 13):
        want = TF.reference(name, which, ins, bh, **TF.scalars(name))
        assert set(outs) == set(want)
        for n in want:
            assert_close_rel(outs[n], want[n], TOL_CPU[dtype], f'{name} {bh} {which} {n}')


@pytest.mark.parametrize('bh', ['zeros', 'periodic'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', ['shift', 'shift2'])
def test_c_backend_shift_is_exact(name, dtype, bh):
    """Weight 1.0 on one neighbour: the output is the shifted input (zeros, or the wrapped values), bit for bit."""
    shape = (5, 6, 7) if TF.ndim(name) == 3 else (6, 7)
    for which, ins, outs in _cpu_run(name, dtype, bh, shape, 14):
        for n, want in TF.reference(name, which, ins, bh).items():
            assert np.array_equal(outs[n], want.astype(dtype)), f'{name} {bh} {which} {n}'


# ------------------------------------------------------------------------------------------- CPU: what the planners say
def _hip(ac, bh='zeros', name='fam', params=None, stub=False):
    k = StencilKernel(ac, boundary_handling=bh, function_name=name, target='gpu', gpu_indexing_params=params)
    return (_plan_helpers().StubKernel if stub else HipStencilKernel)(k)


def _plan_helpers():
    spec = importlib.util.spec_from_file_location('make_march_plan_golden',
                                                  os.path.join(HERE, 'golden', 'make_march_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# family -> direction -> storage type -> 'B' band_plans is not None, 'Z' zsum_plan is not None, 'H' half_ring_ok,
# then the lite fields. As the planners answer at the commit that added these families: band for every fp16 / fp32
# family but the two-field adjoint of ``two_sparse``, zsum for all, the half ring for all fp16 ones; a field is "lite"
# when none of its taps behind the centre plane is off the (0, 0) column.
_ALL = {'f16': 'BZH', 'f32': 'BZ', 'f64': 'Z'}
_NO_BAND = {'f16': 'ZH', 'f32': 'Z', 'f64': 'Z'}
ELIGIBILITY = {
    'shift': {'f': (_ALL, ('u',)), 'b': (_ALL, ())},
    'no_zminus': {'f': (_ALL, ('u',)), 'b': (_ALL, ())},
    'only_zplus': {'f': (_ALL, ('u',)), 'b': (_ALL, ())},
    'plane_only': {'f': (_ALL, ('u',)), 'b': (_ALL, ('diffout',))},
    'x_only': {'f': (_ALL, ('u',)), 'b': (_ALL, ('diffout',))},
    'no_dx': {'f': (_ALL, ()), 'b': (_ALL, ())},
    'upwind': {'f': (_ALL, ('u',)), 'b': (_ALL, ('diffout',))},
    'no_centre': {'f': (_ALL, ()), 'b': (_ALL, ())},
    'q19': {'f': (_ALL, ()), 'b': (_ALL, ())},
    'corners': {'f': (_ALL, ()), 'b': (_ALL, ())},
    'symbol_weight': {'f': (_ALL, ('u',)), 'b': (_ALL, ('diffout',))},
    'two_sparse': {'f': (_ALL, ()), 'b': (_NO_BAND, ())},
}


@pytest.mark.parametrize('name', TF.NAMES_3D)
def test_eligibility_table(name):
    for dtype, key in ((F16, 'f16'), (F32, 'f32'), (F64, 'f64')):
        op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling='zeros')
        for which, ac in _directions(op):
            ir = _hip(ac).ir
            cfg = MarchConfig(VE=16 // np.dtype(dtype).itemsize, ZSUM=True, WS=True, CX=4)
            got = ('B' if band_plans(ir) is not None else '') + ('Z' if zsum_plan(ir, cfg) is not None else '') + \
                ('H' if half_ring_ok(ir, cfg) else '')
            flags, lite = ELIGIBILITY[name][which]
            assert got == flags[key], (name, which, key, got)
            assert tuple(sorted(f.name for f in lite_fields(ir, cfg))) == lite, (name, which, key)


# 2-D family -> view -> (forward, adjoint): the read field is lite. Under 'yx' the field is one plane (nothing lies
# behind it); under 'zy' its rows are the planes, and a tap on a row behind, off the x column, rules the queue out.
LITE_2D = {
    'shift2': {'yx': (True, True), 'zy': (True, False)},
    'x_only2': {'yx': (True, True), 'zy': (True, True)},
    'y_only2': {'yx': (True, True), 'zy': (True, True)},
    'no_centre2': {'yx': (True, True), 'zy': (False, False)},
    'corners2': {'yx': (True, True), 'zy': (False, False)},
}


@pytest.mark.parametrize('view', ['yx', 'zy'])
@pytest.mark.parametrize('name', TF.NAMES_2D)
def test_eligibility_2d(name, view):
    """2-D families: the zsum decomposition applies under both views; which fields are lite, as ``LITE_2D`` records."""
    op = pa.AutoDiffOp(TF.collection(name, 'float32'), boundary_handling='zeros')
    for (which, ac), lite in zip(_directions(op), LITE_2D[name][view]):
        ir = _hip(ac).ir
        cfg = MarchConfig(VE=4, ZSUM=True, VIEW2D=view)
        assert zsum_plan(ir, cfg) is not None
        assert bool(lite_fields(ir, cfg)) == lite, (name, which, view)


# ----------------------------------------------------------------------------------------------- the schedule matrix
TILED = {'CX': 1, 'NR': 2, 'ZC': 4}          # tests/test_periodic_march.py
# (row, what the launch must end on, storage type, shape, tile overrides, boundary handling of the row). 'BAND': None
# stands for the rows per lane ``band_choice`` gives the row length (idle lanes where no whole-wave band exists).
ROWS = [
    ('generic-f32', 'generic', F32, (5, 7, 19), {}, 'zeros'),
    ('generic-f64', 'generic', F64, (5, 7, 19), {}, 'zeros'),
    ('march-reg', 'reg', F32, (7, 11, 72), dict(ZSUM=False, WS=False, CX=1, NR=2, ZC=3), 'zeros'),
    # (rows off 16 bytes: 8-byte plane loads)
    ('march-reg-off16', 'reg', F32, (7, 11, 70), dict(ZSUM=False, WS=False, CX=1, NR=2, ZC=3), 'zeros'),
    ('march-ws', 'ring', F32, (9, 13, 72), dict(ZSUM=False, WS=True, ZC=4), 'zeros'),
    ('zsum-reg', 'zsum', F32, (12, 13, 72), dict(ZSUM=True, WS=False, NW=1, CX=2, NR=3, ZC=5), 'zeros'),
    ('zsum-pk-ar', 'zsum', F32, (12, 13, 72), dict(ZSUM=True, PK=True, AR=True, CX=2, NR=3, ZC=7), 'zeros'),
    ('zsum-ws-f32', 'dma', F32, (12, 13, 72), dict(ZSUM=True, WS=True, D=2, CX=2, WX=2, NR=2, ZC=4), 'zeros'),
    ('zsum-ws-f32-small', 'dma', F32, (4, 5, 8), dict(ZSUM=True, WS=True, D=2, CX=2, WX=2, NR=2, ZC=4), 'zeros'),
    ('zsum-ws-f64', 'dma', F64, (12, 13, 72), dict(ZSUM=True, WS=True, D=2, CX=2, WX=2, NR=2, ZC=4), 'zeros'),
    ('zsum-ws-f64-small', 'dma', F64, (4, 5, 8), dict(ZSUM=True, WS=True, D=2, CX=2, WX=2, NR=2, ZC=4), 'zeros'),
    ('half-ring', 'half', F16, (12, 13, 72), dict(ZSUM=True, WS=True, CX=4, NR=2, D=2, ZC=5), 'zeros'),
    ('band-dpp-f16', 'band', F16, (7, 21, 256), dict(BAND=None, BPAD=0, ZMIN=4, ZMAX=4), 'zeros'),
    ('band-pad-f16', 'band', F16, (7, 21, 256), dict(BAND=None, BPAD=1, ZMIN=4, ZMAX=4), 'zeros'),
    ('band-dpp-f32', 'band', F32, (7, 21, 256), dict(BAND=None, BPAD=0, ZMIN=4, ZMAX=4), 'zeros'),
    ('band-pad-f32', 'band', F32, (7, 21, 256), dict(BAND=None, BPAD=1, ZMIN=4, ZMAX=4), 'zeros'),
    ('band-trim1', 'band', F16, (13, 16, 256), dict(BAND=None, BTRIM=1, ZMIN=5, ZMAX=5), 'zeros'),
    ('band-trim2', 'band', F16, (13, 16, 256), dict(BAND=None, BTRIM=2, ZMIN=5, ZMAX=5), 'zeros'),
    ('band-trim3', 'band', F16, (13, 16, 256), dict(BAND=None, BTRIM=3, ZMIN=4, ZMAX=4), 'zeros'),
    # (dword-aligned row pieces; rows on half dwords; idle lanes in the last compute wave)
    ('band-rows-254', 'band', F16, (5, 9, 254), dict(BAND=None, ZMIN=3, ZMAX=3), 'zeros'),
    ('band-rows-255', 'band', F16, (5, 9, 255), dict(BAND=None, ZMIN=3, ZMAX=3), 'zeros'),
    ('band-rows-520', 'band', F16, (5, 16, 520), dict(BAND=None, ZMIN=3, ZMAX=3), 'zeros'),
    ('periodic-f32-small', 'loader', F32, (2, 2, 8), {}, 'periodic'),
    ('periodic-f32', 'loader', F32, (5, 9, 72), {}, 'periodic'),
    ('periodic-f32-small-tiled', 'loader', F32, (2, 2, 8), TILED, 'periodic'),
    ('periodic-f32-tiled', 'loader', F32, (5, 9, 72), TILED, 'periodic'),
    ('periodic-f16-small', 'loader', F16, (2, 2, 8), {}, 'periodic'),
    ('periodic-f16', 'loader', F16, (5, 9, 72), {}, 'periodic'),
    ('periodic-f16-small-tiled', 'loader', F16, (2, 2, 8), TILED, 'periodic'),
    ('periodic-f16-tiled', 'loader', F16, (5, 9, 72), TILED, 'periodic'),
    ('view-yx', '2d', F32, (40, 72), dict(VIEW2D='yx'), 'zeros'),
    ('view-zy', '2d', F32, (40, 72), dict(VIEW2D='zy'), 'zeros'),
]
# the rows of one z chunk, every other row has at least two: boxes of 2 and 4 planes are below the shortest chunk
# (4 planes per unit of z radius), the periodic default plan keeps its own chunk length (32 planes and more; the
# tiled rows of 5 planes have two chunks), and the 'yx' view of a 2-D field is a single plane
ONE_CHUNK = ('zsum-ws-f32-small', 'zsum-ws-f64-small', 'periodic-f32-small', 'periodic-f32',
             'periodic-f32-small-tiled', 'periodic-f16-small', 'periodic-f16', 'periodic-f16-small-tiled', 'view-yx')
TWO_STORE_KINDS = ('generic', 'zsum', 'dma')            # + the band rows 'band-dpp-*' / 'band-pad-*'


def _cases():
    """(row, family, boundary handling) of the whole matrix."""
    out = []
    for row in ROWS:
        rid, kind, dtype, shape, params, bh = row
        if kind == '2d':
            out += [(row, name, bh) for name in TF.NAMES_2D]
            continue
        for name in TF.FAMILIES:
            out.append((row, name, bh))
            if bh == 'zeros' and name in TF.NONE_FAMILIES:
                out.append((row, name, None))
        if kind in TWO_STORE_KINDS or rid.startswith(('band-dpp', 'band-pad')):
            out += [(row, 'two_sparse', bh), (row, 'two_sparse', None)]
    return out


CASES = _cases()


def _case_id(case):
    return f'{case[0][0]}-{case[1]}-{case[2]}'


def _tile(params, ir, shape, dtype):
    """The row's overrides for one kernel: the band rows ask for the rows per lane that fit the row length and the
    kernel's store count."""
    params = dict(params)
    if 'BAND' in params and params['BAND'] is None:
        es, ns = np.dtype(dtype).itemsize, len(ir.stores)
        choice = band_choice(shape[-1], ns, es) or band_choice(shape[-1], ns, es, idle=True)
        assert choice is not None, (shape, ns, es)
        params['BAND'] = choice[1]
    return params


def _check_variant(kind, name, which, ir, variant, params, shape):
    """The launch took the schedule the row names; where the planner refuses the family there (``ELIGIBILITY``), the
    fallback it took instead."""
    assert variant is not None
    if kind == 'generic':
        assert variant[0] == 'generic', variant
        return
    assert variant[0] == 'march', variant
    cfg = variant[1]
    ws = ws_geometry(ir, cfg)
    if kind == 'band':
        if 'B' not in ELIGIBILITY[name][which][0]['f16']:
            # refused by band_plans (two stencil fields): the zsum schedule of the same kernel
            assert band_plans(ir) is None and cfg.BAND == 0 and cfg.ZSUM, cfg
            return
        assert band_plans(ir) is not None and cfg.BAND == params['BAND'] and cfg.BX == shape[-1], cfg
        for key in ('BPAD', 'BTRIM', 'ZMIN', 'ZMAX'):
            assert key not in params or getattr(cfg, key) == params[key], (key, cfg)
        return
    assert cfg.BAND == 0, cfg
    if kind == 'reg':
        assert not cfg.ZSUM and not cfg.WS and ws is None, cfg
        assert (cfg.CX, cfg.NR) == (params['CX'], params['NR']) and cfg.VE == (4 if shape[-1] % 4 == 0 else 2), cfg
    elif kind == 'ring':
        assert not cfg.ZSUM and cfg.WS and ws is not None and ws['kind'] == 'ring', (cfg, ws)
    elif kind == 'zsum':
        assert cfg.ZSUM and zsum_plan(ir, cfg) is not None, cfg
        assert (cfg.CX, cfg.NR) == (params['CX'], params['NR']) and (cfg.PK or not params.get('PK')), cfg
        assert bool(cfg.AR) or not params.get('AR'), cfg
        if params.get('WS') is False:
            assert not cfg.WS and ws is None, cfg
    elif kind == 'dma':
        assert cfg.ZSUM and cfg.WS and ws is not None and ws['kind'] == 'dma', (cfg, ws)
    elif kind == 'half':
        assert cfg.ZSUM and cfg.WS and half_ring_ok(ir, cfg) and ws is not None and ws['kind'] == 'h', (cfg, ws)
    elif kind == 'loader':
        assert ir.periodic and ws is not None and not (cfg.XM or cfg.XO or cfg.XB), (cfg, ws)
        # fp32 planes go straight into the ring; fp16 planes stay fp16 in it (never an fp32 ring behind a convert)
        half = np.dtype(ir.fields[0].dtype.numpy_dtype) == np.float16
        assert ws['kind'] == ('h' if half else 'dma') and (not half or half_ring_ok(ir, cfg)), (cfg, ws)
    elif kind == '2d':
        assert cfg.VIEW2D == params['VIEW2D'], cfg
    else:
        raise AssertionError(kind)


def _force(kind):
    # (a stencil read at one offset — ``shift`` — would by default stream on one thread per cell)
    return 'generic' if kind == 'generic' else 'march'


def test_matrix_covers_every_family_on_every_row():
    by_row = {}
    for (rid, kind, *_), name, bh in CASES:
        by_row.setdefault(rid, set()).add((name, bh))
    assert set(by_row) == {r[0] for r in ROWS}
    for rid, kind, dtype, shape, params, bh in ROWS:
        names = {n for n, _ in by_row[rid]}
        assert names >= set(TF.FAMILIES if kind != '2d' else TF.NAMES_2D), rid
        if bh == 'zeros' and kind != '2d':
            assert {n for n, b in by_row[rid] if b is None} >= set(TF.NONE_FAMILIES) - {'two_sparse'}, rid


@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_matrix_plans_onto_the_named_schedule(case):
    """No device: with 256-byte-aligned stand-in tensors every launch of the GPU matrix plans onto the schedule its row
    names (or the recorded fallback)."""
    (rid, kind, dtype, shape, params, _), name, bh = case
    G = _plan_helpers()
    op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling=bh)
    for which, ac in _directions(op):
        tile = _tile(params, _hip(ac, bh).ir, shape, dtype)
        hk = _hip(ac, bh, f'fam_{which}', tile, stub=True)
        tensors = G.fake_tensors(hk, shape, 256)
        if kind == 'generic':
            continue                       # (forced at the launch; its plan needs the device's tensors)
        plan = hk._plan_march(tensors, [], shape, 0, None)
        _check_variant(kind, name, which, hk.ir, plan.variant, tile, shape)
        st = plan.statics                  # Z Y X zlo zhi ylo yhi xlo xhi zc ...
        # (the interior-only launches of the 5-plane band rows write 3 planes: one chunk of the 3 that ZMIN asks for)
        one = rid in ONE_CHUNK or (bh is None and rid.startswith('band-rows'))
        assert (st[9] >= st[4] - st[3]) == one, (rid, bh, st)


# ------------------------------------------------------------------------------------------------ CPU: compile sweep
def test_every_family_compiles_on_band_and_ws_schedules():
    """Every family, forward and adjoint, fp16 and fp32, compiles for gfx950 on the band schedule and on the
    warp-specialised zsum schedule. (Cold: about 1 s per kernel, see the commit message.)"""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from pystencils_autodiff_amd.backends.hip_emitter import emit_zsum
    n = 0
    for name in TF.NAMES_3D:
        for dtype in (F16, F32):
            ve = 16 // np.dtype(dtype).itemsize
            op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling='zeros')
            for which, ac in _directions(op):
                hk = _hip(ac, name=f'{name}_{which}')
                if band_plans(hk.ir) is None:
                    assert (name, which) == ('two_sparse', 'b')
                    assert default_march_config(hk.ir, ve, (32, 64, 256), {'BAND': 2}).BAND == 0
                else:
                    cfg = default_march_config(hk.ir, ve, (32, 64, 256), {'BAND': 4 if len(hk.ir.stores) == 1 else 2})
                    assert cfg.BAND > 0, cfg
                    src, kname = hk.source(('march', cfg))
                    assert kname.endswith('_band') and 'band schedule' in src
                    assert len(rt.compile_hip(src)) > 0
                    n += 1
                cfg = default_march_config(hk.ir, ve, (32, 64, 256), dict(ZSUM=True, WS=True))
                assert cfg.ZSUM and cfg.WS and not cfg.BAND and ws_geometry(hk.ir, cfg) is not None, cfg
                assert len(rt.compile_hip(emit_zsum(hk.ir, f'{name}_{which}_zsum', cfg))) > 0
                n += 1
    assert n == 2 * 2 * 2 * len(TF.NAMES_3D) - 2


# ---------------------------------------------------------------------------------------------------------------- GPU
def _torch():
    return pytest.importorskip('torch')


def _seed(shape, extra=''):
    return zlib.crc32(repr((tuple(shape), extra)).encode())


def _compare(name, which, dtype, bh, ins, got, what, **sc):
    """One sweep's outputs against the plain reference ('zeros' / 'periodic') or, interior-only, the oracle's box."""
    from tests.test_gpu_parity import TOL
    shape = next(iter(ins.values())).shape
    ins64 = {n: a.astype(np.float64) for n, a in ins.items()}
    want = TF.reference(name, which, ins64, bh or 'zeros', **sc)
    absr = TF.reference(name, which, ins64, bh or 'zeros', absolute=True, **sc)
    assert set(got) == set(want), (what, sorted(got))
    box = tuple(slice(0, n) for n in shape)
    if bh is None:
        box = tuple(slice(1, n - 1) for n in shape)
        inside = np.zeros(shape, dtype=bool)
        inside[box] = True
    for n, g in got.items():
        w = want[n]
        if bh is None:
            # the written box is the oracle's (pystencils' ghost-layer rule); every cell outside it keeps its NaN
            assert np.isnan(g[~inside]).all(), f'{what} {n}: cells outside the interior box were written'
        # (``assert_cells`` compares with ``>``, which a NaN never satisfies: unwritten cells are looked for here)
        assert not np.isnan(g[box]).any(), \
            f'{what} {n}: {int(np.isnan(g[box]).sum())} cells of the written box are NaN (not stored, or computed so)'
        if name.startswith('shift'):
            assert np.array_equal(g[box], w[box].astype(dtype)), \
                f'{what} {n}: {int((g[box] != w[box].astype(dtype)).sum())} cells are not the shifted input'
        elif dtype == np.float64:
            assert_close_rel(g[box], w[box], TOL[np.float64], f'{what} {n}')
        else:
            assert_cells(g[box], w[box], absr[n][box], TF.n_terms(name, which), dtype, f'{what} {n}')
    return want


def _run_family(row, name, bh):
    """Forward and adjoint of a family on one row of the matrix: seeded inputs in [-1, 1], NaN-filled outputs, the
    schedule asserted, every written cell checked (``symbol_weight``: two launches of the one compiled kernel)."""
    torch = _torch()
    rid, kind, dtype, shape, params, _ = row
    op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling=bh)
    for which, ac in _directions(op):
        tile = _tile(params, _hip(ac, bh).ir, shape, dtype)
        k = StencilKernel(ac, boundary_handling=bh, function_name=f'fam_{which}', target='gpu',
                          gpu_indexing_params=tile).compile()
        ins = _draw([f.name for f in k.ir.fields_read], shape, dtype, _seed(shape, which))
        assert sorted(ins) == sorted(_input_names(name, which))
        tins = {n: torch.from_numpy(a).cuda() for n, a in ins.items()}
        for beta in (TF.BETAS if name == 'symbol_weight' else (None,)):
            sc = TF.scalars(name, beta)
            outs = {f.name: torch.full(shape, float('nan'), dtype=getattr(torch, np.dtype(dtype).name), device='cuda')
                    for f in k.ir.fields_written}
            k(**tins, **outs, **sc, force_schedule=_force(kind))
            torch.cuda.synchronize()
            _check_variant(kind, name, which, k.ir, k.last_variant, tile, shape)
            if bh is None:
                assert k.ir.iteration_bounds(shape) == [(1, n - 1) for n in shape]
            ref = OE.evaluate(ac, {n: a.astype(np.float64) for n, a in ins.items()}, sc, boundary_handling=None) \
                if bh is None else None
            want = _compare(name, which, dtype, bh, ins, {n: t.cpu().numpy() for n, t in outs.items()},
                            f'{rid} {name} {which} {bh} {sc}', **sc)
            if ref is not None:            # interior-only: the oracle's own box and values are the plain reference's
                box = tuple(slice(1, n - 1) for n in shape)
                for n, w in want.items():
                    assert_close_rel(ref[n][box], w[box], 1e-14, f'{name} oracle {n}')


@pytest.mark.parametrize('dtype', [F16, F32, F64], ids=['f16', 'f32', 'f64'])
@pytest.mark.parametrize('bh', ['zeros', 'periodic', None])
def test_compare_sees_unwritten_wrong_and_stray_cells(dtype, bh):
    """The GPU check itself, on the plain reference's own values: it passes them, and fails on one cell of the written
    box left at its NaN fill, on one wrong cell, and (interior-only) on one cell written outside the box."""
    shape = (4, 5, 8)
    ins = _draw(['u'], shape, dtype, 3)
    good = TF.reference('upwind', 'f', {'u': ins['u'].astype(np.float64)}, bh or 'zeros')['out'].astype(dtype)
    if bh is None:
        inside = np.zeros(shape, dtype=bool)
        inside[1:-1, 1:-1, 1:-1] = True
        good[~inside] = np.nan
    _compare('upwind', 'f', dtype, bh, ins, {'out': good}, 'self')
    spoilt = [(2, 2, 3, np.nan), (1, 3, 4, good[1, 3, 4] + dtype(0.05))] + ([(0, 2, 3, 0.0)] if bh is None else [])
    for z, y, x, v in spoilt:
        bad = good.copy()
        bad[z, y, x] = v
        with pytest.raises(AssertionError):
            _compare('upwind', 'f', dtype, bh, ins, {'out': bad}, 'self')


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_case_id)
def test_family_on_schedule(case):
    row, name, bh = case
    _run_family(row, name, bh)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,shape,plan', [(F16, (6, 16, 256), 'band'), (F32, (12, 13, 72), 'zsum')],
                         ids=['f16-band', 'f32-zsum'])
@pytest.mark.parametrize('name', ['q19', 'only_zplus', 'upwind'])
def test_family_through_the_op(name, dtype, shape, plan, monkeypatch):
    """The drop-in op (``create_tensorflow_op(backend='torch_native')``), ``apply`` + ``backward``, against the plain
    references: the fp32 box on its default plan, which is the zsum schedule; fp16 rows of 256 on the band schedule,
    asked for with ``PSAD_MARCH=BAND=4`` as in ``test_band_through_the_op`` (a domain this small has too few
    workgroups for the band to be its default, ``BAND_MIN_WG``)."""
    torch = _torch()
    if plan == 'band':
        monkeypatch.setenv('PSAD_MARCH', 'BAND=4')
    op = pa.AutoDiffOp(TF.collection(name, np.dtype(dtype).name), boundary_handling='zeros')
    fn = op.create_tensorflow_op(use_cuda=True, backend='torch_native')
    u = _draw(['u'], shape, dtype, _seed(shape, 'op'))
    d = _draw(['diffout'], shape, dtype, _seed(shape, 'op-grad'))
    ut = torch.from_numpy(u['u']).cuda().requires_grad_(True)
    (out,) = fn.apply(ut)
    out.backward(torch.from_numpy(d['diffout']).cuda())
    torch.cuda.synchronize()
    for k in (op.forward_ast_gpu.compile(), op.backward_ast_gpu.compile()):
        assert k.last_variant[0] == 'march', k.last_variant
        cfg = k.last_variant[1]
        assert (cfg.BAND > 0) if plan == 'band' else (cfg.BAND == 0 and cfg.ZSUM), cfg
    _compare(name, 'f', dtype, 'zeros', u, {'out': out.detach().cpu().numpy()}, f'op {name} forward')
    _compare(name, 'b', dtype, 'zeros', d, {'diffu': ut.grad.cpu().numpy()}, f'op {name} adjoint')
