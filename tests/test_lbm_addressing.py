"""The addressing variants of the HIP lattice kernels (``LatticeKernels._mode``): buffer resources with 32-bit byte
offsets (``buf``) below 2 GiB, plain pointers (``ptr``) from there on, and ``long long`` strides and offsets once an
array (or the force field) reaches 2³¹ − 1 elements.

CPU: the mode selection at its edges, every variant compiled for gfx950, and the argument buffers of ``plan()`` /
``rho_plan()`` against a ``ctypes.Structure`` of the same fields. GPU: every lattice family forced to ``ptr`` at small
shapes, and the modes selected by reach alone on small lattices whose tensors are strided views into one large,
otherwise untouched buffer — each against the family's float64 reference (``oracle/lbm.py`` and torch's reverse mode
through it; the array-roll restatement of ``test_lbm_neighbour_links`` for neighbour links) at the tolerances of the
family's existing GPU test, never against the ``buf`` result."""
import ctypes
import struct
from collections import namedtuple

import numpy as np
import pytest

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from pystencils_autodiff_amd.lbm import _lattice_kernels as LK
from tests import test_lbm as TL
from tests import test_lbm_neighbour_links as TN
from tests.test_native_abi import _is_amdgpu_elf

I31 = 2 ** 31


# =================================================================================================================
# 1a. mode selection
# =================================================================================================================
def _plain_kernels(dtype, **kw):
    return LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.dtype(dtype), False, 'gpu', **kw)


def _rho_kernels(dtype, programs=False, **kw):
    """Kernels of a D2Q9 lattice with a density-weighted wall (id 1: the adjoint takes the second pass and its scratch
    pointer) and, with ``programs``, a link-program wall (id 2). Only their argument tables are read."""
    plain, rho = (1.0, 0.0, 1.0), (1.0, 0.1, 1.0, 0.05, 0.02)
    links = ((plain,) * 9, (plain,) + (rho,) * 8) + (((0.0, 0.0, 0.0),) * 9,) * programs
    progs = (None, None, (None,) + (((), 'c1', ((1, (), '(T)1'),)),) * 8) if programs else None
    K = LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.dtype(dtype), True, 'gpu', links=links, programs=progs, **kw)
    assert K.rho_links and (K.programs is not None) == programs
    return K


def _meta(reach, dtype, last=2):
    """A meta tensor (no memory) of shape (6, 5, 8, last) whose ``_reach`` is exactly ``reach`` elements."""
    import torch
    base = 40 * 5 + 8 * 4 + 7 + 1
    assert (reach - base) % (last - 1) == 0
    t = torch.empty_strided((6, 5, 8, last), (40, 8, 1, (reach - base) // (last - 1)), dtype=getattr(torch, dtype),
                            device='meta')
    assert LK.LatticeKernels._reach(t) == reach
    return t


@pytest.mark.parametrize('dtype,esize', [('float32', 4), ('float64', 8)])
def test_mode_edges(dtype, esize, monkeypatch):
    """``buf`` up to a reach of 2³¹ − esize bytes, ``ptr`` from 2³¹ bytes; ``int`` up to 2³¹ − 2 elements,
    ``long long`` from 2³¹ − 1; the largest of the launch's tensors decides."""
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    K = _plain_kernels(dtype)
    small = _meta(4096, dtype)
    assert K._mode([small, small]) == ('int', 'buf')
    assert K._mode([_meta(I31 // esize - 1, dtype)]) == ('int', 'buf')
    assert K._mode([_meta(I31 // esize, dtype)]) == ('int', 'ptr')
    assert K._mode([small, _meta(I31 // esize, dtype), small]) == ('int', 'ptr')
    assert K._mode([_meta(I31 - 2, dtype)]) == ('int', 'ptr')
    assert K._mode([_meta(I31 - 1, dtype)]) == ('long long', 'ptr')
    assert K._mode([small, _meta(I31 - 1, dtype)]) == ('long long', 'ptr')
    assert K._mode([_meta(2 ** 33, dtype)]) == ('long long', 'ptr')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_mode_env_forces_ptr_only(dtype, monkeypatch):
    """``PSAD_LBM_ADDR=ptr`` forces plain pointers and leaves the index type alone; any other value does nothing."""
    K = _plain_kernels(dtype)
    small, big = _meta(4096, dtype), _meta(I31 - 1, dtype)
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    assert K._mode([small]) == ('int', 'ptr')
    assert K._mode([big]) == ('long long', 'ptr')
    assert K._launch_mode([small, small]) == ('int', 'ptr')
    monkeypatch.setenv('PSAD_LBM_ADDR', 'buf')
    assert K._mode([small]) == ('int', 'buf')
    assert K._mode([big]) == ('long long', 'ptr')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_launch_mode_force_field_widens_idx_only(dtype, monkeypatch):
    """In ``plan()`` a force field (or its adjoint) reaching 2³¹ − 1 elements turns ``idx`` to ``long long``; the
    small pdf arrays stay buffer resources."""
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    K = _plain_kernels(dtype, force_model='guo', force_field=True)
    pdfs = [_meta(4096, dtype)] * 3
    near, far = _meta(I31 - 2, dtype), _meta(I31 - 1, dtype)
    assert K._launch_mode(pdfs) == ('int', 'buf')
    assert K._launch_mode(pdfs, {'force': (near, near)}) == ('int', 'buf')
    assert K._launch_mode(pdfs[:2], {'force': (far, None)}) == ('long long', 'buf')
    assert K._launch_mode(pdfs, {'force': (far, far)}) == ('long long', 'buf')
    assert K._launch_mode(pdfs, {'force': (near, far)}) == ('long long', 'buf')
    assert K._launch_mode([_meta(I31 // 4, dtype)] * 3, {'force': (far, far)}) == ('long long', 'ptr')


# =================================================================================================================
# the lattice families (shared by the compile test and the GPU tests)
# =================================================================================================================
def _ubb_cavity(shape, dtype, target):
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, data_type=dtype)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.5, target=target)
    TL._set_cavity(step, shape)
    return step


def _noslip_channel(stencil, shape, compressible, layout, dtype, target):
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, layout=layout, data_type=dtype)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.3, target=target)
    TL._set_channel(step, shape)
    return step


def _periodic(stencil, shape, compressible, layout, dtype, target):
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, layout=layout, data_type=dtype)
    return lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.3, target=target)


def _force_field_step(stencil, shape, compressible, model, layout, dtype, target):
    D = len(shape)
    F = ps.fields(f'F({D}): {dtype}[{D}D]', layout=layout)
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, force_model=model, force=F, data_type=dtype)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.4, target=target)
    assert step._lattice is not None and [f.name for f in step._additional_fields] == ['F']
    return step


# one small lattice per family for the compile test: (id, builder of a GPU-target step)
COMPILE_FAMILIES = [
    ('periodic-D3Q19-f32', lambda: _periodic('D3Q19', (6, 5, 8), True, 'fzyx', 'float32', 'gpu')),
    ('noslip-D2Q9-f64', lambda: _noslip_channel('D2Q9', (9, 8), False, 'numpy', 'float64', 'gpu')),
    ('ubb-D2Q9-f32', lambda: _ubb_cavity((9, 8), 'float32', 'gpu')),
    ('ubb-rho-D2Q9-f64', lambda: TL._density_cavity('gpu', True)[0]),
    ('pressure-D2Q9-f32', lambda: TL._pressure_channel('D2Q9', (9, 8), True, 'gpu', False, 'float32')[0]),
    ('pressure-D3Q19-f64', lambda: TL._pressure_channel('D3Q19', (7, 6, 5), True, 'gpu', False, 'float64')[0]),
    ('open-D2Q9-mrt-f64', lambda: TN._lattice('open', 'D2Q9', (9, 8), 'gpu', 'float64', 'mrt')[0]),
    ('box-D3Q19-f32', lambda: TN._lattice('box', 'D3Q19', (7, 6, 5), 'gpu', 'float32')[0]),
    ('mixed-D2Q9-f64', lambda: TN._lattice('mixed', 'D2Q9', (9, 8), 'gpu', 'float64')[0]),
    ('guo-D2Q9-f64', lambda: TL._forced('D2Q9', (9, 8), True, 'guo', 'gpu')[0]),
    ('guo-field-D2Q9-f32', lambda: _force_field_step('D2Q9', (9, 8), True, 'guo', 'numpy', 'float32', 'gpu')),
    ('trt-magic-walls-D2Q9-f64', lambda: TL._trt_case('D2Q9', (9, 8), True, 'magic', 'fzyx', True, 'gpu', 'lattice')[0]),
    ('mrt-walls-D2Q9-f32', lambda: TL._mrt_case('D2Q9', (9, 8), True, 'gpu', True, 'float32')[0]),
]


@pytest.mark.parametrize('family', [c[0] for c in COMPILE_FAMILIES])
def test_every_variant_compiles(family):
    """(``int`` / ``long long``) × (``buf`` / ``ptr``) × (main / fix-up where the lattice has link programs): hiprtc
    gives a gfx950 code object with the entry points of the variant."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    K = dict(COMPILE_FAMILIES)[family]()._lattice_kernels()
    assert K.target == 'gpu'
    assert (K.programs is not None) == family.startswith(('pressure', 'open', 'box', 'mixed'))
    sources = set()
    for idx in ('int', 'long long'):
        for addr in ('buf', 'ptr'):
            for fix in ((False, True) if K.programs is not None else (False,)):
                src = K.source(idx, addr, fix=fix)
                assert f'typedef {idx} IDX;' in src
                assert ('raw_buffer_load' in src) == (addr == 'buf')
                sources.add(src)
                code = rt.compile_hip(src, name='psad_lbm.hip')
                assert _is_amdgpu_elf(code)
                names = ['lbm_adj_fix'] if fix else ['lbm_fwd', 'lbm_adj'] + (['lbm_adj_rho'] if K.rho_links else [])
                for nm in names:
                    assert nm.encode() in code
    assert len(sources) == (8 if K.programs is not None else 4)
    # what a build compiles includes the variant of the largest arrays
    assert len(K.build()) == (6 if K.programs is not None else 3)


# =================================================================================================================
# 1c. argument packing
# =================================================================================================================
_CT = {'Q': ctypes.c_uint64, 'q': ctypes.c_int64, 'i': ctypes.c_int32, 'f': ctypes.c_float, 'd': ctypes.c_double}


def _structure(fmt):
    """The kernel's parameter block as the compiler lays it out: the fields of ``fmt`` at natural alignment."""
    return type('Args', (ctypes.Structure,), {'_fields_': [(f'a{i}', _CT[c]) for i, c in enumerate(fmt)]})


def _values(fmt):
    """A distinct value per slot, every byte of it nonzero."""
    vals = []
    for i, c in enumerate(fmt):
        if c in 'Qq':
            vals.append(int.from_bytes(bytes([0x11 + i] * 8), 'little') >> (1 if c == 'q' else 0))
        elif c == 'i':
            vals.append(0x01010101 * (i % 0x7e + 1))
        else:
            vals.append(1.5 + i)
    return vals


def _check_layout(fmt, vals):
    S = _structure(fmt)
    packed = LK._pack(fmt, *vals)
    assert len(packed) == ctypes.sizeof(S) and len(packed) % 8 == 0
    for i in range(len(fmt)):
        assert LK._offset(fmt, i) == getattr(S, f'a{i}').offset, (fmt, i)
    got = S.from_buffer_copy(packed)
    for i, v in enumerate(vals):
        assert getattr(got, f'a{i}') == v, (fmt, i)
    return S, packed


PACK_CASES = [(idx, dtype, which, force, scratch, fix)
              for idx in ('int', 'long long') for dtype in ('float32', 'float64') for which in ('fwd', 'adj')
              for force in (False, True) for scratch in (False, True) for fix in (False, True)
              if not (which == 'fwd' and (scratch or fix))]


@pytest.mark.parametrize('idx,dtype,which,force,scratch,fix', PACK_CASES)
def test_plan_argument_buffer_matches_struct(idx, dtype, which, force, scratch, fix, monkeypatch):
    """The ``fmt`` of ``plan()`` (``'i'`` / ``'q'`` strides, with and without the force field's pointers and strides,
    the scratch pointer and the fix-up tail ``'Qi'``): ``_pack`` and ``_offset`` agree with the C layout in size, every
    field offset and value; ``LaunchPlan.__call__`` patches the leading pointers and ω at those offsets and nothing
    else."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    K = (_rho_kernels if scratch else _plain_kernels)(dtype, **(dict(force_model='guo', force_field=True) if force
                                                                    else {}))
    ntens = 2 if which == 'fwd' else 3
    nptr = ntens + 2 + ((1 if which == 'fwd' else 2) if force else 0) + int(scratch)
    nstr = 4 * ntens + (4 if force else 0)
    # the format of the kernel's own argument table (the scratch pointer: a lattice whose adjoint takes a second pass)
    kernel = which + ('_fix' if fix else '')
    fmt, om_i = K.arg_format(kernel, idx), [a.kind for a in K.table(kernel)].index('rate')
    code = 'i' if idx == 'int' else 'q'
    om_c = 'f' if dtype == 'float32' else 'd'
    assert fmt == 'Q' * nptr + 'iii' + code * nstr + 'q' * ntens + om_c + ('Qi' if fix else '')
    assert fmt[om_i] == om_c and om_i == nptr + 3 + nstr + ntens
    vals = _values(fmt)
    S, packed = _check_layout(fmt, vals)
    # the launch: pointers and ω patched, every other byte as packed
    sent = []
    monkeypatch.setattr(rt, 'launch', lambda fn, grid, block, args, stream, shared_bytes=0: sent.append(
        (fn, grid, block, args, stream)))
    plan = LK.LaunchPlan(1234, 7, packed, nptr, None, LK._offset(fmt, om_i), fmt[om_i])
    new_ptrs = [0xA0A0A0A0A0A0A0A0 + k for k in range(nptr)]
    plan(tuple(new_ptrs), 99, 0.625)
    (fn, grid, block, args, stream), = sent
    assert (fn, grid, block, stream) == (1234, (7,), (256,), 99)
    want = S.from_buffer_copy(packed)
    for k in range(nptr):
        setattr(want, f'a{k}', new_ptrs[k])
    setattr(want, f'a{om_i}', 0.625)
    assert args == bytes(want)
    got = S.from_buffer_copy(args)
    for i, v in enumerate(vals):
        assert getattr(got, f'a{i}') == (new_ptrs[i] if i < nptr else 0.625 if i == om_i else v)
    # without ω the launch keeps the plan's
    plan(tuple(new_ptrs), 99)
    assert getattr(S.from_buffer_copy(sent[-1][3]), f'a{om_i}') == vals[om_i]
    assert plan.template == packed                      # the template itself is never written


@pytest.mark.parametrize('idx', ['int', 'long long'])
@pytest.mark.parametrize('programs', [False, True])
def test_rho_plan_argument_buffer_matches_struct(idx, programs, monkeypatch):
    """``rho_plan()``'s ``fmt`` is what ``lbm_adj_rho`` declares, with and without link programs on the lattice (on
    the HIP target they run in the fix-up kernel: the second pass takes no src / ids slots): layout as the C struct;
    the launch patches the three leading pointers only."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    K = _rho_kernels('float64', programs)
    fmt = K.arg_format('adj_rho', idx)
    code = 'i' if idx == 'int' else 'q'
    assert fmt == 'QQQiii' + code * 4
    assert [a.name for a in K.table('adj_rho')][:3] == ['out', 'nbmask', 'rho_adj']
    vals = _values(fmt)
    S, packed = _check_layout(fmt, vals)
    sent = []
    monkeypatch.setattr(rt, 'launch', lambda fn, grid, block, args, stream, shared_bytes=0: sent.append(args))
    plan = LK.LaunchPlan(1, 3, packed, 3, None, None, None)
    patched = {0: 0xB1B1B1B1B1B1B1B1, 1: 0xB2B2B2B2B2B2B2B2, 2: 0xB3B3B3B3B3B3B3B3}
    plan(tuple(patched[k] for k in range(3)), 5)
    got = S.from_buffer_copy(sent[0])
    for i, v in enumerate(vals):
        assert getattr(got, f'a{i}') == patched.get(i, v)
    want = S.from_buffer_copy(packed)
    for i, v in patched.items():
        setattr(want, f'a{i}', v)
    assert sent[0] == bytes(want)


def test_pack_pads_like_the_compiler():
    """A 4-byte slot before an 8-byte one leaves a hole; the buffer ends on a multiple of 8."""
    assert LK._offset('Qiq', 2) == 16 and LK._offset('Qiiq', 3) == 16 and LK._offset('iiif', 3) == 12
    assert len(LK._pack('Qi', 1, 2)) == 16
    assert LK._pack('iq', 1, 2) == struct.pack('<i4xq', 1, 2)
    with pytest.raises(IndexError):
        LK._offset('Qi', 2)


# =================================================================================================================
# 2. GPU: every family forced to ``ptr``
# =================================================================================================================
Case = namedtuple('Case', 'make f0 g ref gref T tol gtol fscale run op both extra')


def _case(make, f0, g, ref, gref, T, tol, gtol, fscale, run=True, op=True, both=False, extra=None):
    """``tol`` / ``gtol``: bounds of the forward / adjoint error relative to max|``fscale``| (the reference or the
    initial pdfs, as the family's existing test has it) / max|gref|. ``extra``: (force field, its reference adjoint)."""
    return Case(make, f0, g, np.asarray(ref), np.asarray(gref), T, tol, gtol, float(np.abs(np.asarray(fscale)).max()), run,
                op,
                both, extra)


_CASES = {}


def _cached(fn):
    def wrapper(*key):
        k = (fn.__name__,) + key
        if k not in _CASES:
            _CASES[k] = fn(*key)
        return _CASES[k]
    return wrapper


@_cached
def _periodic_case(stencil, shape, compressible, layout, dtype, T=5):
    """``test_lbm_steps_gpu_vs_oracle``: 1e-12 / 1e-5 of max|ref| forward, ten times that of max|gref| adjoint."""
    f0 = TL._init(stencil, shape, compressible)
    g = np.random.default_rng(1).standard_normal(f0.shape)
    ref, gref = TL._oracle_grad(f0, 1.3, T, stencil, compressible, g)
    tol = 1e-12 if dtype == 'float64' else 1e-5
    return _case(lambda: _periodic(stencil, shape, compressible, layout, dtype, 'gpu'), f0, g, ref, gref, T, tol,
                 10 * tol, ref)


@_cached
def _noslip_case(stencil, shape, compressible, layout, dtype):
    """``test_lbm_lattice_schedule_gpu_vs_oracle``: the same bounds, the no-slip channel with its obstacle."""
    import torch
    f0 = TL._init(stencil, shape, compressible, seed=4)
    g = np.random.default_rng(5).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run_walls(ft, 1.3, torch.tensor(TL._channel(shape)), 5, stencil, compressible, xp=torch)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    tol = 1e-12 if dtype == 'float64' else 1e-5
    return _case(lambda: _noslip_channel(stencil, shape, compressible, layout, dtype, 'gpu'), f0, g, ref.detach(),
                 gref, 5, tol, 10 * tol, ref.detach())


@_cached
def _ubb_case(shape, dtype):
    """``test_lbm_lid_driven_cavity_gpu``: 1e-12 / 1e-5 of max|ref|, ten times that of max|gref|."""
    import torch
    T = 8
    wall, vel = TL._cavity(shape)
    f0 = TL._init('D2Q9', shape, True, seed=23)
    g = np.random.default_rng(24).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run_moving_walls(ft, 1.5, torch.tensor(wall), torch.tensor(vel), T, 'D2Q9', True, xp=torch)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    tol = 1e-12 if dtype == 'float64' else 1e-5
    return _case(lambda: _ubb_cavity(shape, dtype, 'gpu'), f0, g, ref.detach(), gref, T, tol, 10 * tol, ref.detach())


@_cached
def _ubb_rho_case(compressible, trt):
    """``test_lbm_density_weighted_ubb_gpu``: 1e-12 of max|f0| forward, 1e-11 of max|gref| adjoint (float64)."""
    import torch
    _, shape, T, wall, vel, w_odd = TL._density_cavity('cpu', compressible, trt)
    f0 = TL._init('D2Q9', shape, compressible, seed=23)
    g = np.random.default_rng(24).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run_moving_walls(ft, 1.3, torch.tensor(wall), torch.tensor(vel), T, 'D2Q9', compressible, xp=torch,
                              density_weighted=True, omega_odd=w_odd)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    return _case(lambda: TL._density_cavity('gpu', compressible, trt)[0], f0, g, ref.detach(), gref, T, 1e-12, 1e-11, f0)


@_cached
def _pressure_case(stencil, shape, compressible, trt, dtype, T=6):
    """``test_lbm_pressure_channel_gpu``: 1e-12 / 2e-5 of max|f0| forward, ten times that of max|gref| adjoint."""
    args = TL._pressure_channel(stencil, shape, compressible, 'cpu', trt)
    f0 = TL._init(stencil, shape, compressible, seed=33)
    g = np.random.default_rng(34).standard_normal(f0.shape)
    ref, gref = TL._pressure_ref(f0, args, stencil, compressible, T, g)
    tol = 1e-12 if dtype == 'float64' else 2e-5
    return _case(lambda: TL._pressure_channel(stencil, shape, compressible, 'gpu', trt, dtype)[0], f0, g, ref, gref, T,
                 tol, 10 * tol, f0)


@_cached
def _links_case(name, stencil, shape, dtype, method, compressible, both=False, T=6):
    """``test_neighbour_links_gpu``: 1e-12 / 1e-11 (float64), 2e-5 / 2e-4 (float32) of max|f0| / max|gref|."""
    step, kinds, w_odd, mrt = TN._lattice(name, stencil, shape, 'cpu', 'float64', method, compressible)
    f0, g, ref, gref = TN._reference(name, stencil, shape, method, compressible, T, kinds, step.boundary_handling.flags,
                                     w_odd, mrt)
    tol, gtol = (1e-12, 1e-11) if dtype == 'float64' else (2e-5, 2e-4)
    return _case(lambda: TN._lattice(name, stencil, shape, 'gpu', dtype, method, compressible)[0], f0, g, ref, gref, T,
                 tol, gtol, f0, both=both)


@_cached
def _force_case(stencil, shape, compressible, model):
    """``test_lbm_force_models_gpu_vs_oracle`` (float64, ``run`` / ``run_backward``): 1e-12 of max|f0|, 1e-11 of
    max|gref|."""
    import torch
    force = (1e-3, -2e-3, 5e-4)[:len(shape)]
    f0 = TL._init(stencil, shape, compressible, seed=5)
    g = np.random.default_rng(6).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run(ft, 1.4, 3, stencil, compressible, xp=torch, force_model=model, force=force)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    return _case(lambda: TL._forced(stencil, shape, compressible, model, 'gpu')[0], f0, g, ref.detach(), gref, 3, 1e-12,
                 1e-11, f0, op=False)


@_cached
def _force_field_case(stencil, shape, compressible, model, layout, dtype, T=3):
    """``test_lbm_force_field_gpu_vs_oracle`` (the timestep op): 1e-12 of max|ref|, 1e-11 of max|gref| and of
    max|dF_ref| (float64). No float32 force test exists: there the bounds of the float32 periodic lattice, 1e-5 and
    1e-4 (the force terms add a handful of operations per cell to the same arithmetic)."""
    import torch
    D = len(shape)
    rng = np.random.default_rng(sum(shape))
    f0 = TL._init(stencil, shape, compressible, seed=9)
    Fv = 1e-3 * rng.standard_normal(shape + (D,))
    g = rng.standard_normal(f0.shape)
    ft, Fr = torch.tensor(f0, requires_grad=True), torch.tensor(Fv, requires_grad=True)
    ref = OL.run(ft, 1.4, T, stencil, compressible, xp=torch, force_model=model,
                 force=tuple(Fr[..., a] for a in range(D)))
    gx, gF = torch.autograd.grad(ref, (ft, Fr), torch.tensor(g))
    tol, gtol = (1e-12, 1e-11) if dtype == 'float64' else (1e-5, 1e-4)
    return _case(lambda: _force_field_step(stencil, shape, compressible, model, layout, dtype, 'gpu'), f0, g,
                 ref.detach(), gx, T, tol, gtol, ref.detach(), run=False, extra=(Fv, gF.numpy()))


@_cached
def _trt_walls_case(stencil, shape, compressible):
    """``test_lbm_trt_gpu_vs_oracle`` with the magic number and walls (float64, ``run`` / ``run_backward``): 1e-12 of
    max|f0|, 1e-11 of max|gref|."""
    import torch
    rr, w_odd, wall = 1.4, OL.trt_odd_rate(1.4), TL._channel(shape)
    f0 = TL._init(stencil, shape, compressible, seed=4)
    g = np.random.default_rng(5).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run_walls(ft, rr, torch.tensor(wall), 3, stencil, compressible, xp=torch, omega_odd=w_odd)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    return _case(lambda: TL._trt_case(stencil, shape, compressible, 'magic', 'fzyx', True, 'gpu', 'lattice')[0], f0, g,
                 ref.detach(), gref, 3, 1e-12, 1e-11, f0, op=False)


@_cached
def _mrt_walls_case(stencil, shape, compressible, dtype):
    """``test_lbm_mrt_gpu_vs_oracle`` (the timestep op): 1e-12 / 2e-5 of max|f0|, ten times that of max|gref|."""
    import torch
    T = 5
    _, wall, A = TL._mrt_case(stencil, shape, compressible, 'cpu', True)
    f0 = TL._init(stencil, shape, compressible, seed=54)
    g = np.random.default_rng(55).standard_normal(f0.shape)
    ft = torch.tensor(f0, requires_grad=True)
    ref = OL.run_walls(ft, None, torch.tensor(wall), T, stencil, compressible, xp=torch, mrt=A)
    (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
    tol = 1e-12 if dtype == 'float64' else 2e-5
    return _case(lambda: TL._mrt_case(stencil, shape, compressible, 'gpu', True, dtype)[0], f0, g, ref.detach(), gref,
                 T, tol, 10 * tol, f0, run=False)


# (id, case builder, arguments, kernels that must have run besides fwd / adj). Cells / 256 on either side of 8 (the
# XCD remap of the entry points has both branches): e.g. D3Q19 (6, 7, 33) is 6 workgroups, D2Q9 (37, 70) is 11.
PTR_CASES = [
    ('periodic-D3Q19-f32', _periodic_case, ('D3Q19', (6, 7, 33), True, 'fzyx', 'float32'), ()),
    ('periodic-D2Q9-f64', _periodic_case, ('D2Q9', (37, 70), True, 'numpy', 'float64'), ()),
    ('noslip-D2Q9-f64', _noslip_case, ('D2Q9', (37, 70), False, 'numpy', 'float64'), ()),
    ('noslip-D3Q19-f32', _noslip_case, ('D3Q19', (10, 9, 35), False, 'fzyx', 'float32'), ()),
    ('ubb-D2Q9-f32', _ubb_case, ((38, 35), 'float32'), ()),
    ('ubb-D2Q9-f64', _ubb_case, ((70, 33), 'float64'), ()),
    ('ubb-rho-D2Q9-f64', _ubb_rho_case, (True, False), ('adj_rho',)),
    ('ubb-rho-trt-D2Q9-f64', _ubb_rho_case, (True, True), ('adj_rho',)),
    ('pressure-D2Q9-f64', _pressure_case, ('D2Q9', (70, 33), True, False, 'float64'), ('adj_fix',)),
    ('pressure-D2Q9-f32', _pressure_case, ('D2Q9', (66, 37), False, True, 'float32'), ('adj_fix',)),
    ('pressure-D3Q19-f64', _pressure_case, ('D3Q19', (20, 12, 10), True, False, 'float64'), ('adj_fix',)),
    ('pressure-D3Q19-f32', _pressure_case, ('D3Q19', (6, 7, 33), True, False, 'float32'), ('adj_fix',)),
] + [(f'links-{c[0]}-{c[1]}-{"x".join(map(str, c[2]))}-{c[3][-2:]}-{c[4]}', _links_case, c, ('adj_fix',))
     for c in TN.GPU_CASES] + [
    # neighbour-link lattices with no GPU run before: asserted in both modes
    ('links-outflow2-D2Q9-f64', _links_case, ('outflow2', 'D2Q9', (66, 5), 'float64', 'srt', True, True), ('adj_fix',)),
    ('links-box-D3Q19-f32', _links_case, ('box', 'D3Q19', (12, 9, 10), 'float32', 'srt', True, True), ('adj_fix',)),
    ('links-slip-D3Q27-f64', _links_case, ('slip', 'D3Q27', (10, 7, 6), 'float64', 'srt', True, True), ('adj_fix',)),
    ('links-open-D2Q9-mrt-f64', _links_case, ('open', 'D2Q9', (34, 9), 'float64', 'mrt', True, True), ('adj_fix',)),
    ('force-simple-D2Q9-f64', _force_case, ('D2Q9', (8, 6), True, 'simple'), ()),
    ('force-guo-D2Q9-f64', _force_case, ('D2Q9', (9, 12), True, 'guo'), ()),
    ('force-guo-D3Q19-f64', _force_case, ('D3Q19', (6, 5, 4), False, 'guo'), ()),
    ('force-field-guo-D2Q9-f64', _force_field_case, ('D2Q9', (9, 7), True, 'guo', 'numpy', 'float64'), ()),
    ('force-field-guo-D3Q19-f64', _force_field_case, ('D3Q19', (5, 5, 4), False, 'guo', 'fzyx', 'float64'), ()),
    ('trt-magic-walls-D2Q9-f64', _trt_walls_case, ('D2Q9', (12, 9), True), ()),
    ('mrt-walls-D2Q9-f64', _mrt_walls_case, ('D2Q9', (66, 40), True, 'float64'), ()),
    ('mrt-walls-D3Q19-f32', _mrt_walls_case, ('D3Q19', (16, 12, 10), True, 'float32'), ()),
]


def _np(t):
    return t.detach().double().cpu().numpy()


def _run_family(case, dtype):
    """T steps and their adjoint on a fresh step, through ``run`` / ``run_backward`` and / or the timestep op; returns
    ({name: array}, the kernels the step's ``LatticeKernels`` loaded)."""
    import torch
    tdt = getattr(torch, dtype)
    step = case.make()
    assert step._lattice is not None
    K = step._lattice_kernels()
    assert K._fns == {} and K._plans == {}
    f0 = torch.tensor(case.f0, dtype=tdt, device='cuda')
    g = torch.tensor(case.g, dtype=tdt, device='cuda')
    out = {}
    if case.run:
        step.set_pdfs(f0)
        step.run(case.T, record=True)
        out['fwd'] = _np(step.pdf_array)
        step.set_adjoint_pdfs(g)
        step.run_backward(case.T)
        out['adj'] = _np(step.adjoint_pdf_array)
    if case.op:
        op = step.create_timestep_op(case.T)
        x = f0.clone().requires_grad_(True)
        xs = [x]
        if case.extra is not None:
            xs.append(torch.tensor(case.extra[0], dtype=tdt, device='cuda', requires_grad=True))
        res = op.apply(*xs)
        res.backward(g)
        out['fwd_op'], out['adj_op'] = _np(res), _np(x.grad)
        if case.extra is not None:
            out['dforce_op'] = _np(xs[1].grad)
    torch.cuda.synchronize()
    assert step._lattice_kernels() is K
    return out, set(K._fns)


def _errors(case, out):
    err = {}
    for k, a in out.items():
        if k.startswith('fwd'):
            err[k] = np.abs(a - case.ref).max() / case.fscale
        elif k.startswith('adj'):
            err[k] = np.abs(a - case.gref).max() / np.abs(case.gref).max()
        else:
            err[k] = np.abs(a - case.extra[1]).max() / np.abs(case.extra[1]).max()
    return err


def _within(case, err):
    return all(e <= (case.tol if k.startswith('fwd') else case.gtol) for k, e in err.items())


@pytest.mark.gpu
@pytest.mark.parametrize('name', [c[0] for c in PTR_CASES])
def test_family_forced_ptr_gpu(name, monkeypatch):
    """Every lattice family with ``PSAD_LBM_ADDR=ptr`` on a freshly built step: T steps and their adjoint vs the
    family's float64 reference at its existing test's bounds; every kernel the step loaded is a ``ptr`` one, the fix-up
    and the density pass among them where the lattice has them. The ``buf`` run of the same step is printed beside it
    (its largest difference to ``ptr``; not asserted equal: three atomic addends may land in any order) and, for the
    lattices no other GPU test runs, held to the same bounds."""
    import torch
    _, build, args, needs = next(c for c in PTR_CASES if c[0] == name)
    case = build(*args)
    dtype = next((a for a in args if a in ('float32', 'float64')), 'float64')
    dev = torch.cuda.current_device()
    res = {}
    for addr in ('buf', 'ptr'):
        if addr == 'ptr':
            monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
        else:
            monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
        out, fns = _run_family(case, dtype)
        # the run took the variant it claims
        assert fns and all(k[1:] == ('int', addr, dev) for k in fns), fns
        assert {k[0] for k in fns} == {'fwd', 'adj'} | set(needs), fns
        res[addr] = out, _errors(case, out)
    (obuf, ebuf), (optr, eptr) = res['buf'], res['ptr']
    diff = max(np.abs(optr[k] - obuf[k]).max() / np.abs(obuf[k]).max() for k in optr)
    print(f'{name} ptr: ' + ', '.join(f'{k} {e:.2e}' for k, e in eptr.items()) + f'; buf: ' +
          ', '.join(f'{k} {e:.2e}' for k, e in ebuf.items()) + f'; max |buf - ptr| / max|buf| {diff:.2e}')
    assert sorted(eptr) == sorted(k for k, on in (('fwd', case.run), ('adj', case.run), ('fwd_op', case.op),
                                                  ('adj_op', case.op), ('dforce_op', case.extra is not None)) if on)
    assert _within(case, eptr), eptr
    if case.both:
        assert _within(case, ebuf), ebuf


# =================================================================================================================
# 3. GPU: the modes a large reach selects, on sparse views
# =================================================================================================================
def _stride64(span, m):
    """The smallest multiple of 64 whose ``m``-fold is at least ``span`` (in integers: these are near 2³¹)."""
    return -(-int(span) // (64 * int(m))) * 64


def _sparse_layout(shape, Q, layout, reach_min):
    """(sizes, strides, distance between two tensors, reach) of a ``[*shape, Q]`` view whose reach is at least
    ``reach_min`` elements through the smallest large stride that is a multiple of 64: ``'planes'`` — spatial strides
    C-contiguous, the components ``S`` apart (the fzyx layout of a huge lattice: ``q·s_q`` is the large term);
    ``'rows'`` — axis 0 ``S`` apart, inside it ``[…][q][x]`` contiguous (``row_interleaved_empty`` of a huge lattice:
    ``y·s_y`` / ``z·s_z`` is the large term)."""
    cells = int(np.prod(shape))
    X = shape[-1]
    if layout == 'planes':
        sp_strides = [int(np.prod(shape[a + 1:])) for a in range(len(shape))]
        base, m = cells, Q - 1
        S = _stride64(reach_min - base, m)
        strides, dist = sp_strides + [S], cells
    else:
        block = int(np.prod(shape[1:-1])) * Q * X           # one index of axis 0: [rest][q][x]
        base, m = block, shape[0] - 1
        S = _stride64(reach_min - base, m)
        mid = [int(np.prod(shape[a + 1:-1])) * Q * X for a in range(1, len(shape) - 1)]
        strides, dist = [S] + mid + [1, X], max(block, cells)
    return tuple(shape) + (Q,), tuple(strides), dist, base + m * S


class _Views:
    """``n`` pdf views of one layout into one uninitialised buffer, ``dist`` elements (at least the lattice's cell
    count) apart; nothing between the views' elements is ever touched."""

    def __init__(self, n, shape, Q, layout, reach_min, dtype, reach_below=None, limit_bytes=9 * 2 ** 30):
        import torch
        sizes, strides, dist, reach = _sparse_layout(shape, Q, layout, reach_min)
        if reach_below is not None:
            # the largest multiple-of-64 stride that keeps the reach below the limit: one step of 64 back
            big = max(strides)
            strides = tuple(s - 64 if s == big else s for s in strides)
            reach -= 64 * ((Q - 1) if layout == 'planes' else (shape[0] - 1))
            assert reach < reach_below <= reach + 64 * max(Q, shape[0])
        assert dist >= int(np.prod(shape)) and max(strides) >= n * dist
        total = (n - 1) * dist + reach
        esize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = total * esize
        assert self.nbytes <= limit_bytes
        free, _ = torch.cuda.mem_get_info()
        if free < 2 * self.nbytes:
            pytest.skip(f'{free / 2 ** 30:.1f} GiB free on the device: the {self.nbytes / 2 ** 30:.1f} GiB buffer of '
                        'this case needs twice its size')
        self.reach = reach
        self.buffer = torch.empty(total, dtype=dtype, device='cuda')
        self.views = [self.buffer.as_strided(sizes, strides, k * dist) for k in range(n)]
        for v in self.views:
            # in bounds, and no two views share an element
            assert v.storage_offset() + LK.LatticeKernels._reach(v) <= total
            assert LK.LatticeKernels._reach(v) == reach

    def release(self):
        import torch
        self.views = self.buffer = None
        torch.cuda.empty_cache()


def _one_step(step, K, src, dst, g, out, f0, gv, extra=None, extra_adj=None):
    src.copy_(f0)
    g.copy_(gv)
    step._fwd(src, dst, extra or {})
    step._bwd(src, g, out, extra or {}, extra_adj or {})
    return _np(dst), _np(out)


SPARSE_LATTICES = {
    'periodic': lambda dtype: _periodic_case('D2Q9', (37, 70), True, 'numpy', dtype, 1),
    'pressure2': lambda dtype: _pressure_case('D2Q9', (38, 35), True, False, dtype, 1),
    'pressure3': lambda dtype: _pressure_case('D3Q19', (6, 7, 33), True, False, dtype, 1),
    'box': lambda dtype: _links_case('box', 'D2Q9', (22, 13), dtype, 'srt', True, False, 1),
}


# (a) just below 2³¹ bytes, (b) at or just above, (c) 2³¹ − 1 elements and more (float32: float64 would need 16 GiB)
SPARSE_CASES = [(kind, lat, layout, dtype)
                for kind in ('a', 'b') for lat, layout in (('periodic', 'planes'), ('pressure2', 'rows'))
                for dtype in ('float32', 'float64')] + \
    [('c', lat, layout, 'float32') for lat in ('periodic', 'pressure3', 'box') for layout in ('planes', 'rows')]


@pytest.mark.gpu
@pytest.mark.parametrize('kind,lattice,layout,dtype', SPARSE_CASES)
def test_large_reach_on_sparse_views_gpu(kind, lattice, layout, dtype):
    """One step and its adjoint (``step._fwd`` / ``step._bwd``) on small lattices whose four pdf tensors are strided
    views into one large uninitialised buffer, so that reach alone selects the variant: (a) (``int``, ``buf``) with
    the largest byte offsets, the record count and the component offsets next to 2³¹; (b) (``int``, ``ptr``) from 2³¹
    bytes; (c) (``long long``, ``ptr``) from 2³¹ − 1 elements, with the fix-up launch of the wall lattices (the
    ``'box'`` lattice's atomic adds go to other cells through 64-bit offsets). ``dst`` and ``out`` read back through
    the views vs the float64 reference of one step, at the bounds of the forced-``ptr`` test."""
    import torch
    case = SPARSE_LATTICES[lattice](dtype)
    assert case.T == 1
    tdt = getattr(torch, dtype)
    esize = 4 if dtype == 'float32' else 8
    step = case.make()
    K = step._lattice_kernels()
    shape, Q = tuple(case.f0.shape[:-1]), case.f0.shape[-1]
    reach_min, below, want = {'a': (I31 // esize, I31 // esize, ('int', 'buf')),
                              'b': (I31 // esize, None, ('int', 'ptr')),
                              'c': (I31 - 1, None, ('long long', 'ptr'))}[kind]
    V = _Views(4, shape, Q, layout, reach_min, tdt, reach_below=below)
    try:
        src, dst, g, out = V.views
        if kind == 'a':
            assert I31 - 64 * esize * max(Q, shape[0]) <= V.reach * esize < I31
        else:
            assert V.reach >= reach_min
        assert K._mode([src, dst]) == want and K._mode([src, g, out]) == want
        got, gout = _one_step(step, K, src, dst, g, out, torch.tensor(case.f0, dtype=tdt, device='cuda'),
                              torch.tensor(case.g, dtype=tdt, device='cuda'))
        torch.cuda.synchronize()
        dev = torch.cuda.current_device()
        fns = set(K._fns)
        assert fns == {(w,) + want + (dev,) for w in ('fwd', 'adj') + (('adj_fix',) if K.programs is not None else ())}
        assert (K.programs is not None) == (lattice != 'periodic')
        err = {'fwd': np.abs(got - case.ref).max() / case.fscale,
               'adj': np.abs(gout - case.gref).max() / np.abs(case.gref).max()}
        print(f'{kind} {lattice} {layout} {dtype} {want} buffer {V.nbytes / 2 ** 30:.2f} GiB: forward {err["fwd"]:.2e}, '
              f'adjoint {err["adj"]:.2e}')
        assert _within(case, err), err
    finally:
        src = dst = g = out = None
        V.release()


@pytest.mark.gpu
def test_far_force_field_widens_idx_gpu():
    """(d) A D2Q9 ``'guo'`` force field whose two components lie 2³¹ elements apart (``force`` and ``dforce`` two views
    of equal strides into one buffer) beside small contiguous pdfs: (``long long``, ``buf``). ``dst``, ``out`` and the
    accumulated ``dforce`` vs the float64 reference of one step."""
    import torch
    dtype, shape = 'float32', (37, 70)
    case = _force_field_case('D2Q9', shape, True, 'guo', 'numpy', dtype, 1)
    step = case.make()
    K = step._lattice_kernels()
    V = _Views(2, shape, 2, 'planes', I31 - 1, torch.float32)
    try:
        force, dforce = V.views
        force.copy_(torch.tensor(case.extra[0], dtype=torch.float32, device='cuda'))
        dforce.zero_()
        src = torch.tensor(case.f0, dtype=torch.float32, device='cuda')
        g = torch.tensor(case.g, dtype=torch.float32, device='cuda')
        dst, out = torch.empty_like(src), torch.empty_like(src)
        assert K._launch_mode([src, dst], {'force': (force, None)}) == ('long long', 'buf')
        assert K._launch_mode([src, g, out], {'force': (force, dforce)}) == ('long long', 'buf')
        step._fwd(src, dst, {'F': force})
        step._bwd(src, g, out, {'F': force}, {step._adjoint_name(step._force_field): dforce})
        torch.cuda.synchronize()
        dev = torch.cuda.current_device()
        assert set(K._fns) == {('fwd', 'long long', 'buf', dev), ('adj', 'long long', 'buf', dev)}
        err = _errors(case, {'fwd': _np(dst), 'adj': _np(out), 'dforce': _np(dforce)})
        print(f'd force field {shape} {dtype} buffer {V.nbytes / 2 ** 30:.2f} GiB: ' +
              ', '.join(f'{k} {e:.2e}' for k, e in err.items()))
        assert _within(case, err), err
    finally:
        force = dforce = None
        V.release()
