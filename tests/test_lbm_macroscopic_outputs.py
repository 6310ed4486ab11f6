"""Per-step density and velocity outputs of the time-step op: ``create_timestep_op(T, macroscopic_outputs=k)`` returns
``(pdfs, rho, vel)`` with ρ and u of the states k, 2k, …, written by the lattice kernels that compute those states, and
its backward takes their gradients as seeds of the adjoint kernels.

Reference: ``oracle/lbm.py``'s streaming and collision in torch float64, one step at a time (``test_lbm_omega_field.
_reference`` / ``test_lbm_smagorinsky._reference`` with T = 1), ρ and u of every state by the plain moment formulas
written out HERE (``_moments``), and torch's reverse mode through the loss

    Σ_t ⟨a_t, ρ_t⟩ + ⟨b_t, u_t⟩ + ⟨c, f_T⟩

with fixed-seed random a, b, c (a, b zeroed on obstacle cells on the reference side: the kernels emit 0 there)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from tests import test_lbm_omega_field as TO
from tests import test_lbm_smagorinsky as TS
from tests.test_lbm import _init

OMEGA = 1.7
CS = 0.2
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), 'golden')


# --- the reference ---------------------------------------------------------------------------------------------
def _moments(f, stencil, compressible, fm=None, force=None):
    """ρ = Σ_i f_i, u = (Σ_i c_i f_i + F/2 under Guo) (/ρ for a compressible rule) of plain pdfs ``f`` (torch)."""
    import torch
    dirs = OL.SETS[stencil][0]
    rho = f.sum(-1)
    u = []
    for a in range(len(dirs[0])):
        m = sum(c[a] * f[..., i] for i, c in enumerate(dirs) if c[a])
        if fm == 'guo':
            m = m + force[a] / 2
        u.append(m / rho if compressible else m)
    return rho, torch.stack(u, -1)


def _reference_states(f, W, T, stencil, compressible, method, fm, force, walls, cs):
    """The states 1 … T (plain pdfs) from state 0 ``f``: one oracle step at a time."""
    states = []
    for _ in range(T):
        if cs is not None:
            f = TS._reference(f, W, 1, stencil, compressible, method, fm, force, walls)
        else:
            f = TO._reference(f, W, 1, stencil, compressible, method, fm, force, walls)
        states.append(f)
    return states


# --- the step --------------------------------------------------------------------------------------------------
def _make_step(stencil, shape, compressible, target, dtype, method, fm, force_kind, layout, field, zc, cs, walls,
               schedule='lattice'):
    D = len(shape)
    F = ps.fields(f'F({D}): {dtype}[{D}D]') if force_kind == 'field' else None
    force = F if F is not None else TO.FORCE[D] if fm is not None else None
    rule, _ = TS._rule(stencil, compressible, dtype, method, fm, force, layout, field, zc, cs)
    with TO._schedule_env(schedule):
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target=target,
                                                relaxation_rate=None if field else OMEGA)
    assert (step._lattice is not None) == (schedule == 'lattice')
    ref_walls = None if walls is None else TS._set_walls(step, shape, walls)
    return step, ref_walls, force


_REFS = {}


def _case(stencil, shape, compressible=True, target='cpu', dtype='float64', method='srt', fm=None, force_kind=None,
          layout='fzyx', field=False, zc=False, cs=None, walls=None, T=4, k=1, seed=11, seeds='all', pdf_grad=True):
    """The observed time-step op against the reference: (got, reference) pairs of ``out``, ``rho``, ``vel``, ``gx``
    (``gW``, ``gF``) as float64 CPU tensors. ``seeds``: 'all', or 'obstacle' (a, b nonzero on obstacle cells only)."""
    import torch
    D, n = len(shape), T // k
    step, ref_walls, force = _make_step(stencil, shape, compressible, target, dtype, method, fm, force_kind, layout,
                                        field, zc, cs, walls)
    names = [f.name for f in step._additional_fields]
    assert names == [nm for nm, on in (('F', force_kind == 'field'), ('omega_f', field)) if on]
    op = step.create_timestep_op(T, macroscopic_outputs=k)
    if cs is not None:
        # (the Smagorinsky tests' states: the strain norm stays away from zero)
        (f0, W, c), Fv = TS._inputs(stencil, shape, compressible, seed, field), None
    else:
        f0, W, c, Fv = TO._inputs(stencil, shape, compressible, seed, force_kind == 'field')
    rng = np.random.default_rng(seed + 100)
    a, b = rng.standard_normal((n,) + shape), rng.standard_normal((n,) + shape + (D,))
    wall = None if ref_walls is None else np.asarray(ref_walls[1], bool)
    if seeds == 'obstacle':
        a, b = a * wall, b * wall[..., None]
    wts = np.array([float(v) for v in OL.SETS[stencil][1]])
    dev = 'cuda' if target == 'gpu' else 'cpu'
    tdt = getattr(torch, dtype)
    cdt = torch.float64 if dtype == 'float64' else torch.float32            # the observables' type
    x = torch.tensor(f0 - wts if zc else f0, dtype=tdt, device=dev, requires_grad=True)
    Wt = torch.tensor(W, dtype=tdt, device=dev, requires_grad=True) if field else None
    Ft = torch.tensor(Fv, dtype=tdt, device=dev, requires_grad=True) if force_kind == 'field' else None
    extras = [t for t in (Ft, Wt) if t is not None]                         # sorted by name: F, omega_f
    # (the velocity's adjoint in the layout the op returns, component-first: read in place)
    ct, at, bt = torch.tensor(c, dtype=tdt, device=dev), torch.tensor(a, dtype=cdt, device=dev), \
        torch.tensor(np.moveaxis(b, -1, 1).copy(), dtype=cdt, device=dev).permute(0, *range(2, D + 2), 1)
    out, rho, vel = op.apply(x, *extras)
    assert tuple(rho.shape) == (n,) + shape and tuple(vel.shape) == (n,) + shape + (D,)
    assert rho.dtype == cdt and vel.dtype == cdt and rho.is_contiguous()
    assert vel.permute(0, D + 1, *range(1, D + 1)).is_contiguous()          # component-first storage
    assert n == 0 or tuple(bt.stride()) == tuple(vel.stride())
    torch.autograd.backward([out, rho, vel] if pdf_grad else [rho, vel], [ct, at, bt] if pdf_grad else [at, bt])
    key = (stencil, shape, compressible, dtype, method, fm, force_kind, field, zc, cs, walls, T, k, seed, seeds,
           pdf_grad)
    if key not in _REFS:
        # (the reference runs on the inputs as the kernels see them: rounded to the pdf dtype)
        xr = x.detach().double().cpu().requires_grad_()
        Wr = Wt.detach().double().cpu().requires_grad_() if field else None
        Fr = Ft.detach().double().cpu().requires_grad_() if Ft is not None else None
        rw = None if ref_walls is None else (ref_walls[0],) + tuple(torch.tensor(v) for v in ref_walls[1:])
        rforce = tuple(Fr[..., d] for d in range(D)) if Fr is not None else force
        Wref = Wr if field else OMEGA if cs is not None else torch.full(shape, OMEGA, dtype=torch.float64)
        states = _reference_states(xr + torch.tensor(wts) if zc else xr, Wref, T, stencil, compressible, method, fm,
                                   rforce, rw, cs)
        fluid = torch.ones(shape, dtype=torch.bool) if wall is None else torch.tensor(~wall)
        mom = [_moments(states[j * k - 1], stencil, compressible, fm, rforce) for j in range(1, n + 1)]
        rho_r = torch.stack([torch.where(fluid, r, torch.zeros_like(r)) for r, _ in mom]) if n else \
            torch.zeros((0,) + shape, dtype=torch.float64)
        vel_r = torch.stack([torch.where(fluid[..., None], u, torch.zeros_like(u)) for _, u in mom]) if n else \
            torch.zeros((0,) + shape + (D,), dtype=torch.float64)
        loss = (at.double().cpu() * rho_r).sum() + (bt.double().cpu() * vel_r).sum()
        if pdf_grad:
            loss = loss + (ct.double().cpu() * states[-1]).sum()
        ins = [t for t in (xr, Fr, Wr) if t is not None]
        grads = torch.autograd.grad(loss, ins)
        _REFS[key] = (states[-1].detach() - (torch.tensor(wts) if zc else 0), rho_r.detach(), vel_r.detach(),
                      [g.detach() for g in grads])
    out_r, rho_r, vel_r, grads = _REFS[key]
    res = dict(out=(out.detach().double().cpu(), out_r), rho=(rho.detach().double().cpu(), rho_r),
               vel=(vel.detach().double().cpu(), vel_r), gx=(x.grad.double().cpu(), grads[0]))
    for nm, t, g in zip(('gF', 'gW') if Ft is not None else ('gW',), extras, grads[1:]):
        res[nm] = (t.grad.double().cpu(), g)
    res.update(step=step, wall=wall, inputs=(x, extras, ct, at, bt), op=op)
    return res


def _check(res, tol, gtol):
    for name in ('out', 'rho', 'vel', 'gx', 'gW', 'gF'):
        if name in res:
            got, ref = res[name]
            t = gtol if name.startswith('g') else tol
            err, scale = float((got - ref).abs().max()), float(ref.abs().max())
            print(f'{name}: max error {err:.3e} of max {scale:.3e} (ratio {err / scale:.3e}, bound {t:.0e})')
            assert scale > 0 and err <= t * scale, (name, err, scale)
    if res.get('wall') is not None and 'rho' in res:
        w = res['wall']
        assert w.any() and float(res['rho'][0][:, w].abs().max()) == 0.0 and float(res['vel'][0][:, w].abs().max()) == 0.0
        assert float(res['rho'][0][:, ~w].abs().min()) > 0.0


# --- CPU -------------------------------------------------------------------------------------------------------
CPU = {
    'D2Q9': dict(stencil='D2Q9', shape=(9, 7)),
    'D2Q9-incompressible': dict(stencil='D2Q9', shape=(9, 7), compressible=False),
    'D3Q19': dict(stencil='D3Q19', shape=(5, 4, 6)),
    'trt-magic': dict(stencil='D2Q9', shape=(9, 7), method='trt-magic'),
    'mrt': dict(stencil='D2Q9', shape=(9, 7), method='mrt'),
    'guo-constant': dict(stencil='D2Q9', shape=(9, 7), fm='guo', force_kind='const'),
    'simple-constant': dict(stencil='D2Q9', shape=(9, 7), fm='simple', force_kind='const'),
    'guo-field': dict(stencil='D2Q9', shape=(9, 7), fm='guo', force_kind='field'),
    'guo-field-incompressible': dict(stencil='D2Q9', shape=(9, 7), compressible=False, fm='guo', force_kind='field'),
    'omega-field': dict(stencil='D2Q9', shape=(9, 7), field=True),
    'smagorinsky': dict(stencil='D2Q9', shape=(9, 7), cs=CS),
    'zero-centred': dict(stencil='D2Q9', shape=(9, 7), zc=True),
    'noslip-channel': dict(stencil='D2Q9', shape=(12, 9), walls='channel'),
    'pressure-channel': dict(stencil='D2Q9', shape=(12, 9), walls='pressure'),
    'numpy-layout': dict(stencil='D2Q9', shape=(9, 7), layout='numpy'),
}


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('name', list(CPU))
def test_macroscopic_outputs_cpu_vs_reference(name, k):
    """The C lattice kernels, float64, T = 4: pdfs, ρ_t, u_t at 1e-13 and the gradients (pdfs, ``dω``, ``dF``) at 1e-12
    of the maximum."""
    res = _case(**CPU[name], k=k)
    _check(res, 1e-13, 1e-12)
    kw = CPU[name]
    assert ('gW' in res) == bool(kw.get('field')) and ('gF' in res) == (kw.get('force_kind') == 'field')
    if name == 'pressure-channel':
        K = res['step']._lattice_kernels()
        assert K.programs is not None and K.link_pass           # link programs inline plus the second pass


def test_force_field_gets_the_direct_term():
    """Guo with a force field: u reads F directly, so a loss on u alone at the LAST state (no step after it carries
    the seed back to F through the pdfs) has ``dF = dvel / (2ρ)`` exactly there."""
    res = _case(**CPU['guo-field'], T=1, k=1, pdf_grad=False)
    _check(res, 1e-13, 1e-12)
    x, extras, ct, at, bt = res['inputs']
    # (the seed reaches F through the step's collision and directly: the direct part is b / (2ρ), most of dF)
    direct = bt[0].double() / (2 * res['rho'][1][0][..., None])
    assert float(direct.abs().max()) > 0.1 * float(res['gF'][1].abs().max())


def test_obstacle_cells_hold_zero_and_ignore_seeds():
    """ρ = u = 0 exactly in obstacle cells (``_check``), and a seed placed only on obstacle cells changes no gradient:
    bitwise the gradient of the same op without observable gradients."""
    import torch
    res = _case(**CPU['noslip-channel'], seeds='obstacle')
    _check(res, 1e-13, 1e-12)
    x, extras, ct, at, bt = res['inputs']
    assert float(at.abs().max()) > 0 and float(bt.abs().max()) > 0
    seeded = x.grad.clone()
    x.grad = None
    out, rho, vel = res['op'].apply(x)
    out.backward(ct)
    assert torch.equal(seeded, x.grad)


def test_steps_not_a_multiple_of_k():
    """T = 5, k = 2: n = 2, the states 2 and 4."""
    res = _case(**CPU['D2Q9'], T=5, k=2)
    assert res['rho'][0].shape[0] == 2 and res['op'].observed_states == (2, 4)
    _check(res, 1e-13, 1e-12)
    res = _case(**CPU['D2Q9'], T=2, k=3)
    assert res['rho'][0].shape[0] == 0 and res['vel'][0].shape == (0, 9, 7, 2)
    _check({k: v for k, v in res.items() if k not in ('rho', 'vel')}, 1e-13, 1e-12)


@pytest.mark.parametrize('name', ['D2Q9', 'noslip-channel', 'omega-field'])
def test_default_op_and_none_gradients_are_todays(name):
    """``macroscopic_outputs=None`` is today's op (one tensor); the observed op's pdfs are bitwise the plain op's; and
    with ``grad_rho`` / ``grad_vel`` None its gradients are bitwise the plain op's."""
    import torch
    kw = CPU[name]
    step, _, _ = _make_step(kw['stencil'], kw['shape'], True, 'cpu', 'float64', 'srt', None, None, 'fzyx',
                            kw.get('field', False), False, None, kw.get('walls'))
    f0, W, c, _ = TO._inputs(kw['stencil'], kw['shape'], True, 5)
    got = {}
    for mo in ('default', None, 1):
        x = torch.tensor(f0, requires_grad=True)
        ex = [torch.tensor(W, requires_grad=True)] if kw.get('field') else []
        op = step.create_timestep_op(3) if mo == 'default' else step.create_timestep_op(3, macroscopic_outputs=mo)
        out = op.apply(x, *ex)
        if mo == 1:
            assert isinstance(out, tuple) and len(out) == 3
            out = out[0]
        assert torch.is_tensor(out)
        out.backward(torch.tensor(c))
        got[mo] = [out.detach()] + [t.grad for t in [x] + ex]
    for mo in (None, 1):
        for p, q in zip(got['default'], got[mo]):
            assert torch.equal(p, q), mo


def test_loss_on_observables_only():
    """No pdf gradient arrives: the adjoint starts from zero and the seeds."""
    res = _case(**CPU['noslip-channel'], pdf_grad=False)
    _check(res, 1e-13, 1e-12)


def test_gradient_in_another_layout_gets_a_copy():
    """A velocity gradient that does not have the returned view's strides (here: contiguous ``[n, *domain, D]``) and a
    float32 density gradient give the same result as the in-place ones."""
    import torch
    res = _case(**CPU['D2Q9'])
    x, extras, ct, at, bt = res['inputs']
    op = res['op']

    class Relayout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v):
            return v.clone()

        @staticmethod
        def backward(ctx, g):
            return g.contiguous().clone()               # contiguous in [n, *domain, D]: not the op's layout
    first = x.grad.clone()
    x.grad = None
    out, rho, vel = op.apply(x)
    v2 = Relayout.apply(vel)
    torch.autograd.backward([out, rho, v2], [ct, at, bt])
    assert torch.equal(first, x.grad)


def test_end_to_end_trajectories_equal_the_getter_values():
    """``create_end_to_end_op(macroscopic_outputs=True)``: groups of two steps observed at their ends; the trajectories
    equal the getter op's values on the same states, and the four existing attributes are those of the default path."""
    import torch
    shape = (9, 7)
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=OMEGA, target='cpu')
    rng = np.random.default_rng(1)
    rho = torch.tensor(1 + 0.01 * rng.standard_normal(shape))
    vel = torch.tensor(0.03 * rng.standard_normal(shape + (2,)), requires_grad=True)
    r = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1, macroscopic_outputs=True)
    plain = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1)
    assert not hasattr(plain, 'density_trajectory')
    for nm in ('input_pdf_tensor', 'output_pdf_tensor', 'output_density_tensor', 'output_velocity_tensor'):
        assert torch.equal(getattr(r, nm), getattr(plain, nm)), nm
    first = step.create_end_to_end_op(2, vel, rho, num_times_steps_without_save=1)
    assert tuple(r.density_trajectory.shape) == (2,) + shape and tuple(r.velocity_trajectory.shape) == (2,) + shape + (2,)
    for j, e in enumerate((first, plain)):
        for got, ref in ((r.density_trajectory[j], e.output_density_tensor),
                         (r.velocity_trajectory[j], e.output_velocity_tensor)):
            assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    # differentiable through the trajectory: against the getter chain
    (g1,) = torch.autograd.grad((r.velocity_trajectory ** 2).sum(), vel)
    (g2,) = torch.autograd.grad((first.output_velocity_tensor ** 2).sum() + (plain.output_velocity_tensor ** 2).sum(),
                                vel)
    assert float((g1 - g2).abs().max()) <= 1e-12 * float(g2.abs().max())


def test_rule_off_the_lattice_schedule_raises():
    step, _, _ = _make_step('D2Q9', (6, 5), True, 'cpu', 'float64', 'srt', None, None, 'fzyx', False, False, None,
                            None, schedule='autodiffop')
    assert step._lattice is None
    with pytest.raises(NotImplementedError, match='lattice schedule'):
        step.create_timestep_op(2, macroscopic_outputs=True)
    step2, _, _ = _make_step('D2Q9', (6, 5), True, 'cpu', 'float64', 'srt', None, None, 'fzyx', False, False, None, None)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='macroscopic_outputs'):
            step2.create_timestep_op(2, macroscopic_outputs=bad)


# --- the sources -----------------------------------------------------------------------------------------------
def _golden_module():
    spec = importlib.util.spec_from_file_location('make_lattice_macroscopic_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_lattice_macroscopic_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_macroscopic_sources_pinned():
    """Every emitted source of the density / velocity variant is the pinned one (C, HIP ``int`` / ``long long`` ×
    ``buf`` / ``ptr``, fix-up modules where there are programs), and differs from the plain source."""
    mod = _golden_module()
    with open(os.path.join(GOLDEN_DIR, 'lattice_macroscopic_source_sha.json')) as fh:
        golden = json.load(fh)
    shas = mod.shas()
    assert sorted(shas) == sorted(golden)
    assert [k for k in golden if shas[k] != golden[k]] == []
    assert any(k.endswith('-fix') for k in golden) and any('/float16/' in k for k in golden)
    K = mod.kernels('D2Q9-srt-periodic', 'float32', 'gpu')
    assert hashlib.sha256(K.source().encode()).hexdigest() not in golden.values()
    assert K.source(macro=False) == K.source() and 'rho_out' not in K.source()


def test_argument_table_carries_the_group():
    """The new arguments are one group of the one table: the pointers after every other pointer, the strides after
    every other stride; the plain tables are unchanged."""
    mod = _golden_module()
    for name, npt in (('D2Q9-srt-periodic', 4), ('D2Q9-srt-periodic-incompressible-zc', 2)):
        K = mod.kernels(name, 'float64', 'gpu')
        plain, macro = K.table('adj'), K.table('adj', macro=True)
        assert [a for a in macro if a.group != 'macro'] == list(plain)
        assert all(a.group != 'macro' for a in plain)
        grp = [a for a in macro if a.group == 'macro']
        assert [a.name for a in grp if a.kind == 'pointer'] == ['rho_out', 'vel_out', 'drho', 'dvel'][-npt:]
        assert [a.name for a in grp if a.kind == 'stride'] == ['r_z', 'r_y', 'r_x', 'v_c', 'v_z', 'v_y', 'v_x']
        ptrs = [a.name for a in macro if a.kind == 'pointer']
        assert ptrs[-npt:] == [a.name for a in grp if a.kind == 'pointer']
        fwd = [a.name for a in K.table('fwd', macro=True) if a.group == 'macro' and a.kind == 'pointer']
        assert fwd == ['rho_out', 'vel_out']
        assert all('double*' in a.decl for a in grp if a.kind == 'pointer')
    Kh = mod.kernels('D2Q9-srt-periodic', 'float16', 'gpu')
    assert all('float*' in a.decl for a in Kh.table('fwd', macro=True) if a.group == 'macro' and a.kind == 'pointer')


@pytest.mark.parametrize('fix', [False, True])
@pytest.mark.parametrize('addr', ['buf', 'ptr'])
@pytest.mark.parametrize('idx', ['int', 'long long'])
def test_macroscopic_sources_compile(monkeypatch, idx, addr, fix):
    """The variant of a walled family with link programs (a FixedDensity channel, float32): (``int`` / ``long long``)
    × (``buf`` / ``ptr``) × (main / fix-up) compile to gfx950 code objects."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from tests.test_native_abi import _is_amdgpu_elf
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    K = _golden_module().kernels('D2Q9-srt-pressure', 'float32', 'gpu')
    assert K.programs is not None
    src = K.source(idx, addr, fix=fix, macro=True)
    assert src.count('rho_out[rc] = mo_r;') == 1 and src.count('const float mo_s = drho[rc]') == 1
    code = rt.compile_hip(src, name='psad_lbm.hip')
    assert _is_amdgpu_elf(code)
    for nm in (['lbm_adj_fix'] if fix else ['lbm_fwd', 'lbm_adj']):
        assert nm.encode() in code


# --- GPU -------------------------------------------------------------------------------------------------------
GPU_F64 = {
    'D2Q9-channel': dict(stencil='D2Q9', shape=(37, 70), walls='channel'),
    'D3Q19-guo-field': dict(stencil='D3Q19', shape=(20, 17, 70), fm='guo', force_kind='field'),
    'D3Q27-channel': dict(stencil='D3Q27', shape=(10, 9, 66), walls='channel', k=2),
    'D2Q9-omega-field-smagorinsky': dict(stencil='D2Q9', shape=(37, 70), field=True, cs=CS),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GPU_F64))
def test_macroscopic_outputs_gpu_vs_reference(name):
    """The HIP lattice kernels in float64, T = 3, at 1e-12 (forward values) and 1e-11 (gradients)."""
    res = _case(**dict(dict(T=3), **GPU_F64[name]), target='gpu')
    _check(res, 1e-12, 1e-11)


@pytest.mark.gpu
def test_macroscopic_outputs_fixup_launch_gpu():
    """The pressure channel, D2Q9 (70, 33): the listed cells' seeds enter through the fix-up launch only (the main
    launch returns before it loads ``g`` there); the gradient at the listed cells matches, and a second backward is
    bitwise equal."""
    import torch
    shape = (70, 33)
    res = _case('D2Q9', shape, target='gpu', walls='pressure', T=3)
    _check(res, 1e-12, 1e-11)
    step = res['step']
    cells = step._cells_arg()
    assert cells is not None and int(cells.numel()) > 0
    listed = np.zeros(int(np.prod(shape)), bool)
    listed[cells.cpu().numpy()] = True
    listed = torch.tensor(listed.reshape(shape))
    got, ref = res['gx']
    assert float((got[listed] - ref[listed]).abs().max()) <= 1e-11 * float(ref.abs().max())
    x, extras, ct, at, bt = res['inputs']
    again = []
    for _ in range(2):
        x.grad = None
        torch.autograd.backward(list(res['op'].apply(x)), [ct, at, bt])
        again.append(x.grad.clone())
    assert torch.equal(again[0], again[1]) and torch.equal(again[0].double().cpu(), got)


@pytest.mark.gpu
def test_macroscopic_outputs_ptr_addressing_bitwise_gpu(monkeypatch):
    """``PSAD_LBM_ADDR=ptr``: bitwise equal to ``buf`` in float64."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    a = _case('D2Q9', (37, 70), target='gpu', walls='channel', T=3)
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    b = _case('D2Q9', (37, 70), target='gpu', walls='channel', T=3)
    assert {k[2] for k in b['step']._lattice_kernels()._fns} == {'ptr'}
    assert {k[2] for k in a['step']._lattice_kernels()._fns} == {'buf'}
    assert any(k[-1] == 'macro' for k in b['step']._lattice_kernels()._fns)
    for k in ('out', 'rho', 'vel', 'gx'):
        assert torch.equal(a[k][0], b[k][0]), k


@pytest.mark.gpu
def test_macroscopic_outputs_gpu_against_cpu():
    """The HIP and the C kernels agree on one float64 case at 1e-12."""
    kw = dict(stencil='D2Q9', shape=(37, 70), walls='channel', T=3)
    a, b = _case(**kw, target='gpu'), _case(**kw, target='cpu')
    for k in ('out', 'rho', 'vel', 'gx'):
        err, scale = float((a[k][0] - b[k][0]).abs().max()), float(b[k][0].abs().max())
        print(f'{k}: HIP against C {err:.3e} of {scale:.3e}')
        assert err <= 1e-12 * scale, k


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape', [('D2Q9', (64, 48)), ('D3Q19', (20, 17, 70))])
def test_macroscopic_outputs_float32_gpu(stencil, shape):
    """float32, no-slip channel with an obstacle, T = 3: pdfs within 1e-5 and the pdf gradient within 1e-4 of the
    maximum (the existing bounds); u is a quotient of cancelling sums, so the error of ρ, u and of every gradient
    against the float64 reference is at most 4× the error of the same reference run in float32 on the CPU on the same
    inputs. Measured on an MI355X: see DESIGN.md, "Density and velocity outputs"."""
    import torch
    T = 3
    res = _case(stencil, shape, target='gpu', dtype='float32', walls='channel', T=T)
    x, extras, ct, at, bt = res['inputs']
    wall = torch.tensor(res['wall'])
    x32 = x.detach().cpu().requires_grad_()
    states = _reference_states(x32, torch.full(shape, OMEGA, dtype=torch.float32), T, stencil, True, 'srt', None, None,
                               ('noslip', wall), None)
    mom = [_moments(s, stencil, True) for s in states]
    rho32 = torch.stack([torch.where(~wall, r, torch.zeros_like(r)) for r, _ in mom])
    vel32 = torch.stack([torch.where(~wall[..., None], u, torch.zeros_like(u)) for _, u in mom])
    loss = (at.cpu() * rho32).sum() + (bt.cpu() * vel32).sum() + (ct.cpu() * states[-1]).sum()
    (g32,) = torch.autograd.grad(loss, x32)
    cpu32 = dict(out=states[-1].detach(), rho=rho32.detach(), vel=vel32.detach(), gx=g32)
    ratios = {}
    for name in ('out', 'rho', 'vel', 'gx'):
        got, ref = res[name]
        e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu32[name].double() - ref).abs().max())
        ratios[name] = e_gpu / e_cpu
        print(f'{stencil} {name}: error {e_gpu:.3e}, float32 reference {e_cpu:.3e}, ratio {ratios[name]:.3f} (bound 4)')
    print(f'{stencil}: worst ratio {max(ratios.values()):.3f}')
    _check({k: res[k] for k in ('out', 'gx')}, 1e-5, 1e-4)
    w = res['wall']
    assert float(res['rho'][0][:, w].abs().max()) == 0.0 and float(res['vel'][0][:, w].abs().max()) == 0.0
    for name in ('rho', 'vel', 'gx'):
        got, ref = res[name]
        assert float((got - ref).abs().max()) <= 4 * float((cpu32[name].double() - ref).abs().max()), name


@pytest.mark.gpu
@pytest.mark.parametrize('zc', [False, True], ids=['plain', 'zero-centred'])
def test_macroscopic_outputs_fp16_gpu(zc):
    """float16 pdfs, float32 outputs, D2Q9 (64, 48), periodic, T = 2. The kernel sums the post-collision values before
    their cast to half; the stored state holds each of them rounded once (relative error ≤ 2⁻¹¹). So per cell, against
    the moments of the kernels' OWN stored states s (state 1: the one-step op's output, the same launch; state 2: this
    op's output), ``|ρ − Σ_i s_i| ≤ Q·2⁻¹¹·max_i|s_i| + (fp32 term)`` and the same for each momentum component ``ρ u_a``
    against ``Σ_i c_ia s_i``; the fp32 term is 4× the largest difference of that moment between one reference step from
    the kernels' stored previous state run in float32 and in float64 on the CPU."""
    import torch
    stencil, shape, T, Q = 'D2Q9', (64, 48), 2, 9
    step, _, _ = _make_step(stencil, shape, True, 'gpu', 'float16', 'srt', None, None, 'fzyx', False, zc, None, None)
    wts = torch.tensor([float(v) for v in OL.SETS[stencil][1]], dtype=torch.float64)
    f0 = _init(stencil, shape, True, seed=12)
    x = torch.tensor(f0 - wts.numpy() if zc else f0, dtype=torch.float16, device='cuda')
    out, rho, vel = step.create_timestep_op(T, macroscopic_outputs=1).apply(x)
    assert rho.dtype == torch.float32 and vel.dtype == torch.float32 and out.dtype == torch.float16
    s1, _, _ = step.create_timestep_op(1, macroscopic_outputs=1).apply(x)
    stored = [x.cpu(), s1.cpu(), out.cpu()]
    dirs = OL.SETS[stencil][0]
    worst = 0.0
    for t in (1, 2):
        s = stored[t].double()
        plain = s + wts if zc else s
        rho_s, _ = _moments(plain, stencil, False)
        mom_s = _moments(s, stencil, False)[1]                  # Σ_i c_i s_i (Σ_i c_i w_i = 0)
        prev = stored[t - 1]
        nxt = {}
        for dt in (torch.float32, torch.float64):
            p = prev.to(dt) + (wts.to(dt) if zc else 0)
            f = TO._reference(p, torch.full(shape, OMEGA, dtype=dt), 1, stencil, True)
            nxt[dt] = _moments(f, stencil, False)
        term_r = 4 * float((nxt[torch.float32][0].double() - nxt[torch.float64][0]).abs().max())
        term_m = 4 * float((nxt[torch.float32][1].double() - nxt[torch.float64][1]).abs().max())
        half = Q * 2.0 ** -11 * s.abs().max(-1).values
        got_r = rho[t - 1].double().cpu()
        got_m = got_r[..., None] * vel[t - 1].double().cpu()
        e_r, e_m = (got_r - rho_s).abs(), (got_m - mom_s).abs().max(-1).values
        worst = max(worst, float((e_r / (half + term_r)).max()), float((e_m / (half + term_m)).max()))
        print(f'state {t} zero_centered={zc}: rho {float((e_r / (half + term_r)).max()):.3f}, momentum '
              f'{float((e_m / (half + term_m)).max()):.3f} of the bound (fp32 terms {term_r:.2e}, {term_m:.2e}; '
              f'half terms ≥ {float(half.min()):.2e})')
        assert bool((e_r <= half + term_r).all()) and bool((e_m <= half + term_m).all())
        assert len(dirs) == Q
