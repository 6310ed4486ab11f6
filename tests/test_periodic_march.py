"""``boundary_handling='periodic'`` on the march schedules: the LDS-DMA loader fills the plane image from wrapped
source offsets (``hip_emitter.loader._ws_piece_offsets``), out-of-domain planes are the kernel's own far planes or the z-slab
halos (``ws_plane_base``).

CPU part: which kernels ``schedule()`` sends to ``'march'``, which launches the planner gives an LDS-DMA loader
(stub tensors of ``tests/golden/make_march_plan_golden.py``), that every such source compiles for gfx950, that the emit
functions without a periodic form refuse a periodic IR, and the sources' SHA-256
(``tests/golden/emit_periodic_sha.json``, regenerate: ``python tests/test_periodic_march.py``).

GPU part: parity through the op against the float64 oracle. The oracle has no periodic mode: every input is wrap-padded
by the stencil radius on all three axes, evaluated under ``'zeros'`` and cropped (``periodic_reference``); Σ|terms| for
``conftest.assert_cells`` comes from the same construction on |inputs|."""
import hashlib
import importlib.util
import json
import os
from dataclasses import replace

import numpy as np
import pytest

torch = pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))
SHA_PATH = os.path.join(HERE, 'golden', 'emit_periodic_sha.json')


def _plan_helpers():
    spec = importlib.util.spec_from_file_location('make_march_plan_golden',
                                                  os.path.join(HERE, 'golden', 'make_march_plan_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def radius2_asym(dtype='float32'):
    from pystencils_autodiff_amd import ps
    u, out = ps.fields(f'u, out: {dtype}[3d]')
    return ps.AssignmentCollection({out.center: 0.3 * u[2, 0, 0] - 0.7 * u[0, -2, 0] + 0.25 * u[0, 1, -2]
                                    + 0.2 * u[-1, 0, 1]})


def _builders():
    from pystencils_autodiff_amd import workloads as W
    # name -> (builder, numpy storage dtype, stencil radius)
    return {'asym7_f32': (W.asym_7pt, np.float32, 1),
            'diffusion7_f32': (W.diffusion_7pt, np.float32, 1),
            'diffusion7_f64': (lambda: W.diffusion_7pt(dtype='float64'), np.float64, 1),
            'stencil27_f16': (W.stencil_27pt, np.float16, 1),
            'varcoef_f32': (W.varcoef_diffusion_7pt, np.float32, 1),
            'radius2_f32': (radius2_asym, np.float32, 2)}


KERNELS = tuple(_builders())
SMALL = {1: (2, 2, 8), 2: (3, 3, 8)}        # the smallest box of whole 16-byte rows a radius allows
TILED = {'CX': 1, 'NR': 2, 'ZC': 4}


def _op(name, params=None):
    import pystencils_autodiff_amd as pa
    builder = _builders()[name][0]
    kw = {'gpu_indexing_params': params} if params else {}
    return pa.AutoDiffOp(builder(), boundary_handling='periodic', **kw)


def periodic_reference(collection, inputs, r):
    """{output: float64 array}: ``collection`` on wrap-padded ``inputs`` under 'zeros', cropped by ``r``."""
    from oracle import evaluate as OE
    padded = {n: np.pad(np.asarray(a, dtype=np.float64), r, mode='wrap') for n, a in inputs.items()}
    out = OE.evaluate(collection, padded, boundary_handling='zeros')
    return {n: a[r:-r, r:-r, r:-r] for n, a in out.items()}


def assert_periodic_cells(actual, collection, inputs, r, storage, what):
    """``conftest.assert_cells`` per output against ``periodic_reference``: defaults for linear stencils,
    ``slack = 4·degree`` for polynomial ones (the ``assert_cells_linear`` rule)."""
    import sympy as sp

    from tests.conftest import abs_poly, assert_cells
    ref = periodic_reference(collection, inputs, r)
    ac, deg = abs_poly(collection, max_degree=4)
    absr = periodic_reference(ac, {n: np.abs(np.asarray(a, dtype=np.float64)) for n, a in inputs.items()}, r)
    nt = max(len(sp.Add.make_args(a.rhs)) for a in ac.main_assignments)
    for name, got in actual.items():
        assert_cells(got, ref[name], absr[name], nt, storage, f'{what} {name}', slack=4.0 * max(1, deg))
    return ref


# ------------------------------------------------------------------------------------------------------ CPU: schedule
def _hip_kernel(assignments, name='k', params=None, stub=False):
    from pystencils_autodiff_amd.backends.hip_kernel import HipStencilKernel
    from pystencils_autodiff_amd.backends.kernel_ir import StencilKernel
    cls = _plan_helpers().StubKernel if stub else HipStencilKernel
    return cls(StencilKernel(assignments, boundary_handling='periodic', function_name=name, target='gpu',
                             gpu_indexing_params=params))


@pytest.mark.parametrize('name', KERNELS)
def test_schedule_is_march_for_3d_scalar_periodic_stencils(name):
    op = _op(name)
    assert _hip_kernel(op.forward_assignments).schedule() == 'march'
    assert _hip_kernel(op.backward_assignments).schedule() == 'march'


def test_schedule_stays_generic_outside_the_march_class():
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import ps
    from tests.test_lbm import _periodic_case
    op2d = pa.AutoDiffOp(_periodic_case(), boundary_handling='periodic')
    assert _hip_kernel(op2d.forward_assignments).schedule() == 'generic'
    assert _hip_kernel(op2d.backward_assignments).schedule() == 'generic'
    u, o = ps.fields('u(2), o(2): float32[3d]')
    vec = ps.AssignmentCollection({o.center(0): u[1, 0, 0](0) - u[0, 0, -1](1),
                                   o.center(1): u[0, -1, 0](0) + u.center(1)})
    assert _hip_kernel(vec).schedule() == 'generic'
    u, o = ps.fields('u, o: float32[3d]')
    assert _hip_kernel(ps.AssignmentCollection({o[1, 0, 0]: u.center})).schedule() == 'generic'      # push_periodic
    u, v, o = ps.fields('u, v, o: float32[3d]')
    assert _hip_kernel(ps.AssignmentCollection({o.center: u[1, 0, 0] + 0.5 * v[0, -1, 0]})).schedule() == 'generic'


# --------------------------------------------------------------------------------------------------------- CPU: plans
def _shapes(name):
    return [(5, 33, 264), SMALL[_builders()[name][2]], (70, 9, 16)]


def _stub_kernels(name, params=None):
    op = _op(name)
    return [(which, _hip_kernel(asg, f'{name}_{which}', params, stub=True))
            for which, asg in (('fwd', op.forward_assignments), ('bwd', op.backward_assignments))]


def _march_plans():
    """(row key, stub kernel, plan) of every periodic launch of the matrix: the three default-tile shapes and the
    overridden small tile, forward and adjoint of every kernel."""
    G = _plan_helpers()
    out = []
    for name in KERNELS:
        for params, shapes in ((None, _shapes(name)), (TILED, [(9, 10, 72)])):
            for which, hk in _stub_kernels(name, params):
                for shape in shapes:
                    plan = hk._plan_march(G.fake_tensors(hk, shape, 256), [], shape, 0, None)
                    out.append((f'{name}/{which} {G.shape_text(shape)} {G.kv_text(params or {})}'.rstrip(), hk, plan))
    return out


def test_periodic_plans_end_on_an_lds_dma_loader():
    from pystencils_autodiff_amd.backends.hip_emitter import ws_geometry
    for key, hk, plan in _march_plans():
        assert plan.variant[0] == 'march', key
        cfg = plan.variant[1]
        assert ws_geometry(hk.ir, cfg) is not None, key
        assert cfg.BAND == 0 and not cfg.XM and cfg.XO == 0 and not cfg.XB, key


def test_rows_or_pointers_off_16_bytes_plan_generic_and_refuse_halos():
    G = _plan_helpers()
    (_, hk), _ = _stub_kernels('asym7_f32')
    shape = (5, 9, 70)                                   # fp32 rows of 280 bytes
    assert hk._plan_march(G.fake_tensors(hk, shape, 256), [], shape, 0, None).variant[0] == 'generic'
    shape = (5, 33, 264)
    assert hk._plan_march(G.fake_tensors(hk, shape, 4), [], shape, 0, None).variant[0] == 'generic'     # class 2
    assert hk._plan_march(G.fake_tensors(hk, shape, 16), [], shape, 0, None).variant[0] == 'march'
    ts, halos = G.real_tensors(hk, (5, 9, 70), 0, 'both')
    with pytest.raises(ValueError, match='row pitch of 280 bytes'):
        hk._plan_march(ts, halos, (5, 9, 70), 0, None)
    ts, halos = G.real_tensors(hk, shape, 1, 'both')     # every tensor one element (4 bytes) into its buffer
    with pytest.raises(ValueError, match='4-byte aligned'):
        hk._plan_march(ts, halos, shape, 0, None)
    with pytest.raises(ValueError, match='4-byte aligned'):
        hk._plan_march(G.fake_tensors(hk, shape, 4), [], shape, 0, (0, 2))
    with pytest.raises(ValueError, match='radius'):
        hk._plan_march(G.fake_tensors(hk, (1, 9, 16), 256), [], (1, 9, 16), 0, None)


# ------------------------------------------------------------------------------------------------------- CPU: sources
def periodic_rows():
    """{row key: SHA-256 of the emitted source} over ``_march_plans``, and the distinct sources with their hiprtc
    options."""
    rows, sources = {}, {}
    for key, hk, plan in _march_plans():
        src = hk.source(plan.variant)[0]
        rows[key] = hashlib.sha256(src.encode()).hexdigest()
        sources[rows[key]] = (src, hk.options(plan.variant))
    return rows, sources


def test_periodic_sources_compile_and_match_the_pinned_hashes():
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    rows, sources = periodic_rows()
    for src, options in sources.values():
        assert 'wrapped piece' in src and '0x7ffffff0' in src
        assert rt.compile_hip(src, options)
    with open(SHA_PATH) as fh:
        want = json.load(fh)
    assert list(rows) == list(want)
    bad = [k for k in want if want[k] != rows[k]]
    assert not bad, f'{len(bad)} periodic sources differ from tests/golden/emit_periodic_sha.json: {bad[:10]}'


def test_emit_functions_without_a_periodic_form_refuse_a_periodic_kernel():
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import workloads as W
    from pystencils_autodiff_amd.backends import hip_emitter as E
    from pystencils_autodiff_amd.backends.hip_band import emit_band
    from pystencils_autodiff_amd.backends.kernel_ir import StencilKernel
    from pystencils_autodiff_amd.backends.march_plan import default_march_config
    (_, hk), _ = _stub_kernels('asym7_f32')
    with pytest.raises(ValueError, match='periodic'):
        E.emit_zsum(hk.ir, 'k', E.MarchConfig(VE=4, ZSUM=True))            # register prefetch, no loader
    with pytest.raises(ValueError, match='periodic'):
        E.emit_march(hk.ir, 'k', E.MarchConfig(VE=4))
    ws = hk._plan_march(_plan_helpers().fake_tensors(hk, (5, 33, 264), 256), [], (5, 33, 264), 0, None).variant[1]
    assert E.emit_zsum(hk.ir, 'k', ws)
    for bad in (dict(XM=True), dict(XB=True)):
        with pytest.raises(ValueError, match='periodic'):
            E.emit_zsum(hk.ir, 'k', replace(ws, **bad))
    (_, vk), _ = _stub_kernels('varcoef_f32')
    with pytest.raises(ValueError, match='periodic'):
        E.emit_march(vk.ir, 'k', E.MarchConfig(VE=4, NT_STORE=True))
    (_, bk), _ = _stub_kernels('stencil27_f16')
    zeros = StencilKernel(pa.AutoDiffOp(W.stencil_27pt(), boundary_handling='zeros').forward_assignments,
                          boundary_handling='zeros', function_name='z', target='gpu')
    band = default_march_config(zeros.ir, 8, (768, 768, 768))
    assert band.BAND and emit_band(zeros.ir, 'k', band)
    with pytest.raises(ValueError, match='periodic'):
        emit_band(bk.ir, 'k', band)


# ------------------------------------------------------------------------------------------------ GPU: through the op
def _inputs(op, shape, dt, seed):
    """numpy inputs U(0, 1) by forward input name, gradients U(−1, 1) by forward output name, in the storage type."""
    rng = np.random.default_rng(seed)
    x = {f.name: rng.uniform(0, 1, shape).astype(dt) for f in op.forward_input_fields}
    g = {f.name: rng.uniform(-1, 1, shape).astype(dt) for f in op.forward_output_fields}
    return x, g


def _apply(op, x, g, view=None):
    """``apply`` + ``backward`` of the op's torch function: ({output: array}, {'diff<input>': array}).
    ``view(array) -> GPU tensor`` places an input (default: a fresh tensor)."""
    fn = op.create_tensorflow_op(use_cuda=True, backend='torch_native')
    place = view or (lambda a: torch.from_numpy(a).cuda())
    ins = [place(x[f.name]).requires_grad_(True) for f in op.forward_input_fields]
    outs = fn.apply(*ins)
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    torch.autograd.backward(list(outs), [torch.from_numpy(g[f.name]).cuda() for f in op.forward_output_fields])
    torch.cuda.synchronize()
    got = {f.name: o.detach().cpu().numpy() for f, o in zip(op.forward_output_fields, outs)}
    grads = {'diff' + f.name: t.grad.cpu().numpy() for f, t in zip(op.forward_input_fields, ins)}
    return got, grads


def _check(op, name, shape, x, g, got, grads):
    _, dt, r = _builders()[name]
    assert_periodic_cells(got, op.forward_assignments, x, r, dt, f'{name} {shape} fwd')
    bwd_in = {**x, **{'diff' + n: a for n, a in g.items()}}
    assert_periodic_cells(grads, op.backward_assignments, bwd_in, r, dt, f'{name} {shape} bwd')


def _variants(op):
    return op.forward_ast_gpu.compile().last_variant[0], op.backward_ast_gpu.compile().last_variant[0]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['small', 'partial_tiles', 'chunks', 'tiled'])
@pytest.mark.parametrize('name', KERNELS)
def test_periodic_march_parity_through_the_op(name, case):
    """small: every halo piece wraps onto the tile's own cells, planes −1 and Z are one plane. partial_tiles
    (5, 33, 264): a second x tile of 8 cells whose right halo wraps to column 0, a second y tile of one row whose
    upper halo wraps to row 0. chunks (70, 9, 16): at least two z chunks. tiled (9, 10, 72) on CX=1, NR=2, ZC=4:
    interior tile boundaries and wrapped edges on all three axes."""
    _, dt, r = _builders()[name]
    shape = {'small': SMALL[r], 'partial_tiles': (5, 33, 264), 'chunks': (70, 9, 16), 'tiled': (9, 10, 72)}[case]
    op = _op(name, TILED if case == 'tiled' else None)
    x, g = _inputs(op, shape, dt, seed=3)
    got, grads = _apply(op, x, g)
    if case == 'chunks' and op.forward_ast_gpu.compile().last_plan.statics[9] >= shape[0]:
        op = _op(name, {'ZC': 32})                       # the default chunking gave one chunk
        got, grads = _apply(op, x, g)
    assert _variants(op) == ('march', 'march')
    if case in ('chunks', 'tiled'):
        for k in (op.forward_ast_gpu, op.backward_ast_gpu):
            st = k.compile().last_plan.statics           # Z Y X zlo zhi ylo yhi xlo xhi zc ...
            assert st[9] < st[0], st
    _check(op, name, shape, x, g, got, grads)
    if name == 'diffusion7_f64' and case == 'partial_tiles':
        lhs = float(np.vdot(got['out'], g['out']))
        rhs = float(np.vdot(x['u'], grads['diffu']))
        assert abs(lhs - rhs) <= 1e-11 * float(np.abs(g['out']).sum()), (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize('name,shape', [('asym7_f32', (5, 9, 70)), ('stencil27_f16', (5, 9, 66))])
def test_rows_off_16_bytes_stay_generic_and_correct(name, shape):
    op = _op(name)
    x, g = _inputs(op, shape, _builders()[name][1], seed=4)
    got, grads = _apply(op, x, g)
    assert _variants(op) == ('generic', 'generic')
    _check(op, name, shape, x, g, got, grads)


@pytest.mark.gpu
def test_one_op_takes_both_plans_by_pointer_alignment():
    """The same periodic op on a 16-byte-aligned view and on a view 4 bytes into a larger buffer: the march plan, then
    the one-thread-per-cell plan, both within the bound."""
    name, shape = 'asym7_f32', (5, 33, 264)
    op = _op(name)
    x, g = _inputs(op, shape, np.float32, seed=5)
    n = int(np.prod(shape))

    def view(offset):
        def place(a):
            buf = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
            v = buf[offset:offset + n].view(shape)
            v.copy_(torch.from_numpy(a))
            assert v.data_ptr() % 16 == 4 * offset
            return v.detach()
        return place
    got_a, grads_a = _apply(op, x, g, view(0))
    assert op.forward_ast_gpu.compile().last_variant[0] == 'march'
    got_u, grads_u = _apply(op, x, g, view(1))
    assert op.forward_ast_gpu.compile().last_variant[0] == 'generic'
    _check(op, name, shape, x, g, got_a, grads_a)
    _check(op, name, shape, x, g, got_u, grads_u)


if __name__ == '__main__':
    table = periodic_rows()[0]
    with open(SHA_PATH, 'w') as fh:
        json.dump(table, fh, indent=1)
        fh.write('\n')
    print(f'{len(table)} rows -> {SHA_PATH}')
