"""The Smagorinsky subgrid model: ``create_lb_update_rule(..., smagorinsky=C_s)`` — the relaxation rate of a cell is

    ω_eff = 2 / (τ0 + √(τ0² + 18 C_s² q)),   τ0 = 1/ω0,   q = N/ρ (incompressible: N),
    N = √(2 Σ_ab Π_ab²),   Π_ab = Σ_i c_ia c_ib (f_i − feq_i)

of the cell's own pulled pdfs; the lattice kernels evaluate it in the forward and the adjoint cell and carry its chain
factors (``_lattice_source.smagorinsky.smagorinsky_adjoint``).

Reference: ``oracle/lbm.py``'s streaming and ``collide`` with the per-cell tensor ω_eff(fs) computed HERE from the formulas
above (``OL.equilibrium``), in torch float64, and ``torch.autograd.grad`` through T = 3 steps. Every parity test asserts on
the reference's own states, at each step over fluid cells, that the strain norm stays away from zero (min q ≥ 1e-4) and
that the model is exercised (max |ω_eff − ω0| ≥ 1e-4)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import sympy as sp

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from pystencils_autodiff_amd.lbm._lattice_source import LatticeSource
from tests import test_lbm as TL
from tests import test_lbm_neighbour_links as TN
from tests import test_lbm_omega_field as TO
from tests.test_lbm import _channel, _set_channel

CS = 0.2
OMEGA = 1.7
FORCE = TO.FORCE
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), 'golden')


# --- the reference ---------------------------------------------------------------------------------------------
def _omega_eff(fs, W0, stencil, compressible, fm=None, force=None, cs=CS):
    """(ω_eff, q) of the streamed pdfs ``fs`` (torch), per cell, from the issue's formulas."""
    import torch
    dirs = OL.SETS[stencil][0]
    D = len(dirs[0])
    rho = fs.sum(-1)
    u = []
    for a in range(D):
        m = sum(c[a] * fs[..., i] for i, c in enumerate(dirs) if c[a])
        if fm == 'guo':
            m = m + force[a] / 2
        u.append(m / rho if compressible else m)
    n = fs - OL.equilibrium(rho, torch.stack(u, -1), stencil, compressible, xp=torch)
    sq = 0
    for a in range(D):
        for b in range(D):
            Pi = sum(c[a] * c[b] * n[..., i] for i, c in enumerate(dirs) if c[a] * c[b])
            sq = sq + Pi * Pi
    N = torch.sqrt(2 * sq)
    q = N / rho if compressible else N
    tau0 = 1 / W0
    R = torch.sqrt(tau0 * tau0 + 18 * cs * cs * q)
    return 2 / (tau0 + R), q


def _reference(f, W0, T, stencil, compressible, method='srt', fm=None, force=None, walls=None, stats=None):
    """``T`` steps in torch with the per-cell rate ω_eff(fs); ``walls`` as ``test_lbm_omega_field._reference``.
    ``stats``: a list that receives (min q, max |ω_eff − ω0|) over fluid cells of every step."""
    import torch
    for _ in range(T):
        if walls is None:
            fs, keep = OL.stream(f, stencil, torch), None
        elif walls[0] == 'noslip':
            fs, keep = OL.stream_walls(f, stencil, walls[1], torch), walls[1]
        else:
            fs, keep = OL.stream_pressure_walls(f, stencil, walls[1], walls[2], walls[3], compressible, torch), walls[1]
        W, q = _omega_eff(fs, W0, stencil, compressible, fm, force)
        if stats is not None:
            fluid = torch.ones_like(q, dtype=torch.bool) if keep is None else ~keep
            W0d = W0.detach() if torch.is_tensor(W0) else W0
            stats.append((float(q.detach()[fluid].min()), float((W.detach() - W0d).abs()[fluid].max())))
        new = TO._collide(fs, W, stencil, compressible, method, fm, force, torch)
        f = new if keep is None else torch.where(keep.unsqueeze(-1), f, new)
    return f


def _assert_exercised(stats, T):
    assert len(stats) == T
    for t, (qmin, shift) in enumerate(stats):
        print(f'reference step {t}: min q {qmin:.3e}, max |omega_eff - omega0| {shift:.3e}')
        assert qmin >= 1e-4 and shift >= 1e-4, (t, qmin, shift)


# --- the step --------------------------------------------------------------------------------------------------
def _rule(stencil, compressible, dtype='float64', method='srt', fm=None, force=None, layout='fzyx', field=False,
          zero_centered=False, cs=CS):
    D = lbm.LBStencil(stencil).D
    w = ps.fields(f'omega_f: {dtype}[{D}D]') if field else None
    rate = w.center if field else sp.Symbol('omega')
    kw = {}
    if method == 'trt-magic':
        kw = dict(method='trt')
    elif method == 'trt-rate':
        kw = dict(method='trt', relaxation_rates=[rate, TO.ODD_RATE])
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[rate] + [TO.MRT_CONST[k] for k in ('bulk', 'third', 'fourth')])
    if 'relaxation_rates' not in kw:
        kw['relaxation_rate'] = rate
    if fm is not None:
        kw.update(force_model=fm, force=force)
    return lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, layout=layout,
                                     zero_centered=zero_centered, smagorinsky=cs, **kw), w


def _set_walls(step, shape, walls):
    """The walls of ``test_lbm_omega_field._step`` ('channel' / 'pressure') and their reference description."""
    D = len(shape)
    if walls == 'channel':
        _set_channel(step, shape)
        ref = ('noslip', _channel(shape))
    else:
        wall = np.zeros(shape, bool)
        for end in (0, -1):
            step.set_boundary_including_adjoint(lbm.NoSlip(), TN._end(D, 1, end))
            wall[TN._end(D, 1, end)] = True
        inner = TN._end(D, 0, 0, (1,)), TN._end(D, 0, -1, (1,))
        step.set_boundary_including_adjoint(lbm.FixedDensity(TL.RHO_IN, name='inlet'), inner[0])
        step.set_boundary_including_adjoint(lbm.FixedDensity(TL.RHO_OUT, name='outlet'), inner[1])
        pressure, rho_w = np.zeros(shape, bool), np.ones(shape)
        pressure[inner[0]] = pressure[inner[1]] = True
        rho_w[inner[0]], rho_w[inner[1]] = TL.RHO_IN, TL.RHO_OUT
        ref = ('pressure', wall | pressure, pressure, rho_w)
        assert step._lattice_kernels().programs is not None
    assert np.array_equal(step.boundary_handling.flags != 0, ref[1])
    return ref


def _step(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, force=None, layout='fzyx',
          field=False, zero_centered=False, schedule='lattice', walls=None):
    rule, w = _rule(stencil, compressible, dtype, method, fm, force, layout, field, zero_centered)
    with TO._schedule_env(schedule):
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target=target,
                                                relaxation_rate=None if field else OMEGA)
    assert (step._lattice is not None) == (schedule == 'lattice')
    if schedule == 'lattice':
        assert step._lattice_kernels().smagorinsky == CS and step._lattice_kernels().spec.sm == CS
    return step, (None if walls is None else _set_walls(step, shape, walls))


def _inputs(stencil, shape, compressible, seed, field=False):
    """f0 = feq(ρ, u) (1 + 0.05 ξ), ρ = 1 + 0.05 ξ, u = 0.05 ξ, ξ uniform in [−1, 1]; the ω field uniform in
    [0.6, 1.9]; the output adjoint standard normal."""
    rng = np.random.default_rng(seed)
    D, Q = len(shape), len(OL.SETS[stencil][0])
    rho = 1 + 0.05 * rng.uniform(-1, 1, shape)
    u = 0.05 * rng.uniform(-1, 1, shape + (D,))
    f0 = OL.equilibrium(rho, u, stencil, compressible) * (1 + 0.05 * rng.uniform(-1, 1, shape + (Q,)))
    W = rng.uniform(0.6, 1.9, shape) if field else None
    return f0, W, rng.standard_normal(f0.shape)


_CASES = {}


def _case(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, layout='fzyx', field=False,
          zero_centered=False, schedule='lattice', walls=None, T=3, seed=11):
    """The timestep op against the reference (computed once per lattice and shared): (got, reference) pairs of the pdfs
    ``out``, the pdf adjoint ``gx`` and, with an ω field, ``gW``, as float64 CPU tensors."""
    import torch
    D = len(shape)
    force = FORCE[D] if fm is not None else None
    step, ref_walls = _step(stencil, shape, compressible, target, dtype, method, fm, force, layout, field,
                            zero_centered, schedule, walls)
    assert [f.name for f in step._additional_fields] == (['omega_f'] if field else [])
    op = step.create_timestep_op(T)
    f0, W, g = _inputs(stencil, shape, compressible, seed, field)
    wts = np.array([float(v) for v in OL.SETS[stencil][1]])
    dev = 'cuda' if target == 'gpu' else 'cpu'
    tdt = getattr(torch, dtype)
    # (the reference runs on the inputs as the kernels see them: rounded to the pdf dtype)
    x = torch.tensor(f0 - wts if zero_centered else f0, dtype=tdt, device=dev, requires_grad=True)
    Wt = torch.tensor(W, dtype=tdt, device=dev, requires_grad=True) if field else None
    gt = torch.tensor(g, dtype=tdt, device=dev)
    out = op.apply(x, *([Wt] if field else []))
    out.backward(gt)
    key = (stencil, shape, compressible, dtype, method, fm, field, zero_centered, walls, T, seed)
    if key not in _CASES:
        xr = x.detach().double().cpu().requires_grad_()
        Wr = Wt.detach().double().cpu().requires_grad_() if field else None
        rw = None if ref_walls is None else (ref_walls[0],) + tuple(torch.tensor(a) for a in ref_walls[1:])
        stats = []
        ref = _reference(xr + torch.tensor(wts) if zero_centered else xr, Wr if field else OMEGA, T, stencil,
                         compressible, method, fm, force, rw, stats)
        grads = torch.autograd.grad(ref, (xr, Wr) if field else (xr,), gt.double().cpu())
        _CASES[key] = (ref.detach() - (torch.tensor(wts) if zero_centered else 0), [t.detach() for t in grads], stats)
    ref, grads, stats = _CASES[key]
    _assert_exercised(stats, T)
    res = dict(out=(out.detach().double().cpu(), ref), gx=(x.grad.double().cpu(), grads[0]))
    if field:
        res['gW'] = (Wt.grad.double().cpu(), grads[1])
    res['step'], res['walls'], res['inputs'] = step, ref_walls, (x, Wt, gt)
    return res


_check = TO._check


# --- 1. the rule -----------------------------------------------------------------------------------------------
def test_rule_keyword():
    """``smagorinsky=False`` / ``None``: today's rule, assignment for assignment; ``True``: C_s = 0.12; a number or a
    symbol: C_s; anything else a ``ValueError``. The subexpressions have stable names and the main assignments read
    ``omega_eff``."""
    for kw in (dict(), dict(method='trt'), dict(method='mrt', relaxation_rates=[sp.Symbol('omega'), 1.1]),
               dict(force_model='guo', force=(1e-3, 2e-3))):
        plain = lbm.create_lb_update_rule('D2Q9', compressible=True, **kw)
        for off in (False, None):
            rule = lbm.create_lb_update_rule('D2Q9', compressible=True, smagorinsky=off, **kw)
            assert [str(a) for a in rule.all_assignments] == [str(a) for a in plain.all_assignments]
            assert rule.smagorinsky is None
    assert lbm.create_lb_update_rule('D2Q9', smagorinsky=True).smagorinsky == sp.Rational(12, 100)
    assert float(lbm.create_lb_update_rule('D2Q9', smagorinsky=0.2).smagorinsky) == 0.2
    C = sp.Symbol('C_s')
    rule = lbm.create_lb_update_rule('D2Q9', smagorinsky=C)
    assert rule.smagorinsky == C and rule.relaxation_rate == sp.Symbol('omega')
    names = [str(a.lhs) for a in rule.subexpressions]
    assert names[-7:] == ['smag_Pi_00', 'smag_Pi_01', 'smag_Pi_11', 'smag_N', 'smag_q', 'smag_R', 'omega_eff']
    for a in rule.main_assignments:
        assert sp.Symbol('omega_eff') in a.rhs.free_symbols and sp.Symbol('omega') not in a.rhs.free_symbols
    for bad in (0, -1, 'x', 0.0):
        with pytest.raises(ValueError, match='smagorinsky'):
            lbm.create_lb_update_rule('D2Q9', smagorinsky=bad)


# --- 2. CPU: the lattice schedule against the reference ----------------------------------------------------------
#             stencil, shape, compressible, method, force model, layout, walls, ω field, zero-centred
CPU_LATTICE = [('D2Q9', (9, 7), True, 'srt', None, 'fzyx', None, False, False),
               ('D2Q9', (9, 7), False, 'srt', None, 'fzyx', None, False, False),
               ('D2Q9', (12, 9), True, 'srt', None, 'fzyx', 'channel', False, False),
               ('D3Q19', (5, 4, 6), True, 'srt', None, 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'trt-magic', None, 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'trt-rate', None, 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'mrt', None, 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'srt', 'guo', 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'srt', 'simple', 'fzyx', None, False, False),
               ('D2Q9', (9, 7), True, 'srt', None, 'fzyx', None, True, False),
               ('D2Q9', (9, 7), True, 'srt', None, 'fzyx', None, False, True),
               ('D2Q9', (9, 7), True, 'srt', None, 'numpy', None, False, False)]


@pytest.mark.parametrize('stencil,shape,compressible,method,fm,layout,walls,field,zc', CPU_LATTICE)
def test_smagorinsky_lattice_cpu_vs_reference(stencil, shape, compressible, method, fm, layout, walls, field, zc):
    """The C lattice kernels, float64, T = 3 through the timestep op, at 1e-12 (pdfs) and 1e-11 (adjoints) of the
    maximum."""
    res = _case(stencil, shape, compressible, 'cpu', method=method, fm=fm, layout=layout, walls=walls, field=field,
                zero_centered=zc)
    _check(res, 1e-12, 1e-11)
    assert ('gW' in res) == field


# --- 3. the formulas against sympy's Jacobian ------------------------------------------------------------------
@pytest.mark.parametrize('guo', [False, True])
@pytest.mark.parametrize('method', ['srt', 'trt-magic', 'mrt'])
def test_adjoint_formulas_match_the_symbolic_jacobian(method, guo):
    """One adjoint step of the emitted C kernels on a 3×3 periodic lattice against ``Σ_i g_i ∂dst_i/∂f_k`` with sympy's
    Jacobian of the rule's main assignments (subexpressions inlined) at the same numbers: 1e-11 of the maximum."""
    st = lbm.LBStencil('D2Q9')
    shape = (3, 3)
    Fc = FORCE[2] if guo else None
    rule, _ = _rule('D2Q9', True, method=method, fm='guo' if guo else None, force=Fc)
    lhs = {a.lhs for a in rule.all_assignments}
    acc = sorted({x for a in rule.all_assignments for x in a.rhs.atoms(ps.Field.Access)} - lhs, key=str)
    f = [next(a for a in acc if tuple(a.index) == (i,)) for i in range(9)]            # the pulled pdfs src_i(x − c_i)
    assert len(acc) == 9 and all(tuple(int(o) for o in f[i].offsets) == tuple(-c for c in st.directions[i])
                                 for i in range(9))
    om = sp.Symbol('omega')
    # sympy's derivative of every assignment by everything it reads; the total derivative by the pulled pdfs follows by
    # the chain rule through the subexpressions, in their order, on numbers (the inlined 9 × 9 Jacobian is the same
    # function, and takes sympy a minute)
    order = list(rule.subexpressions) + list(rule.main_assignments)
    parts = []
    for a in order:
        reads = sorted((x for x in a.rhs.free_symbols if x in lhs or x in f), key=str)
        parts.append((a.lhs, reads, sp.lambdify(reads + [om], [a.rhs] + [sp.diff(a.rhs, x) for x in reads], 'math')))

    def Jf(*args):
        vals = dict(zip(f, args[:9]))
        grad = {x: np.eye(9)[k] for k, x in enumerate(f)}
        rows = []
        for name, reads, fn in parts:
            r = fn(*[vals[x] for x in reads], args[9])
            vals[name], grad[name] = r[0], sum((d * grad[x] for d, x in zip(r[1:], reads)), np.zeros(9))
            if isinstance(name, ps.Field.Access):
                rows.append(grad[name])
        return np.array(rows)
    f0, _, g = _inputs('D2Q9', shape, True, 5)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA)
    assert step._lattice is not None
    step.set_pdfs(f0)
    step.run(1, record=True)
    step.set_adjoint_pdfs(g)
    step.run_backward(1)
    got = np.array(step.adjoint_pdf_array)
    want = np.zeros_like(f0)
    for y in range(3):
        for x in range(3):
            cell = [((y - c[0]) % 3, (x - c[1]) % 3) for c in st.directions]      # where f_k was pulled from
            Jv = np.array(Jf(*[f0[cell[k] + (k,)] for k in range(9)], OMEGA), dtype=np.float64)
            v = g[y, x] @ Jv
            for k in range(9):
                want[cell[k] + (k,)] = v[k]
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print(f'{method} guo={guo}: max error {err:.3e} of {scale:.3e}')
    assert err <= 1e-11 * scale


# --- 4. the schedules agree ------------------------------------------------------------------------------------
def test_schedules_agree_cpu():
    """The lattice kernels against the rule's AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``, the generic transposed
    derivation through the symbolic square roots)."""
    a = _case('D2Q9', (9, 7), True, 'cpu', schedule='lattice')
    b = _case('D2Q9', (9, 7), True, 'cpu', schedule='autodiffop')
    _check(b, 1e-12, 1e-11)
    _check({k: (a[k][0], b[k][0]) for k in ('out', 'gx')}, 1e-12, 1e-11)


# --- 5. the rest state -----------------------------------------------------------------------------------------
def test_rest_state_has_the_plain_gradient():
    """Uniform ρ = 1, u = 0 (N = 0 in every cell, at every step): the forward result is the plain SRT step's within
    1e-14, and the lattice gradient is finite and the plain rule's within 1e-12 (∂N/∂f is defined as 0 there)."""
    import torch
    shape, T = (8, 6), 2
    wts = np.array([float(v) for v in OL.SETS['D2Q9'][1]])
    f0 = np.broadcast_to(wts, shape + (9,)).copy()
    g = np.random.default_rng(3).standard_normal(f0.shape)
    res = {}
    for cs in (CS, False):
        rule = lbm.create_lb_update_rule('D2Q9', compressible=True, smagorinsky=cs)
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA)
        assert step._lattice is not None
        x = torch.tensor(f0, requires_grad=True)
        out = step.create_timestep_op(T).apply(x)
        out.backward(torch.tensor(g))
        res[cs] = (out.detach().numpy(), x.grad.numpy())
    assert np.isfinite(res[CS][1]).all()
    assert np.abs(res[CS][0] - res[False][0]).max() <= 1e-14
    assert np.abs(res[CS][1] - res[False][1]).max() <= 1e-12 * np.abs(res[False][1]).max()


# --- 6. routing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['float16', 'force-field', 'symbol'])
def test_other_combinations_take_the_autodiffop_schedule(what):
    """float16 pdfs, a per-cell force field and a symbolic C_s run on the rule's AutoDiffOp kernels (C_s from
    ``kernel_params``): ``step._lattice is None``, and one step runs."""
    shape = (6, 5)
    f0, _, _ = _inputs('D2Q9', shape, True, 7)
    wts = np.array([float(v) for v in OL.SETS['D2Q9'][1]])
    extra, params, dtype, zc = {}, None, 'float64', False
    if what == 'float16':
        dtype, zc = 'float16', True
        rule = lbm.create_lb_update_rule('D2Q9', compressible=True, data_type='float16', zero_centered=True,
                                         smagorinsky=CS)
    elif what == 'force-field':
        F = ps.fields('F(2): float64[2D]')
        rule = lbm.create_lb_update_rule('D2Q9', compressible=True, force_model='guo', force=F, smagorinsky=CS)
        extra = {'F': np.full(shape + (2,), 1e-3)}
    else:
        rule = lbm.create_lb_update_rule('D2Q9', compressible=True, smagorinsky=sp.Symbol('C_s'))
        params = {'C_s': CS}
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA,
                                            kernel_params=params)
    assert step._lattice is None
    step.set_pdfs((f0 - wts if zc else f0).astype(dtype))
    step.run(1, extra=extra)
    got = np.asarray(step.pdf_array, dtype=np.float64) + (wts if zc else 0)
    assert np.isfinite(got).all()
    if what == 'symbol':
        import torch
        ref = _reference(torch.tensor(f0), OMEGA, 1, 'D2Q9', True)
        assert np.abs(got - ref.numpy()).max() <= 1e-13 * np.abs(ref.numpy()).max()


def test_forward_before_the_op_is_the_ops_kernel(monkeypatch):
    """A forward run on the AutoDiffOp schedule compiles the rule alone (no transposed derivation yet); the op built
    afterwards takes that very kernel as its forward kernel, so what it recorded of its launches stays visible."""
    monkeypatch.setenv('PSAD_LBM_LATTICE', '0')
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(6, 5), relaxation_rate=1.3, target='cpu')
    f0, _, g = _inputs('D2Q9', (6, 5), True, 9)
    step.set_pdfs(f0)
    step.run(2, record=True)
    assert step._autodiff_op is None and step._forward_only is not None
    ran = step._forward_only.compile()
    assert step.autodiff_op.forward_ast_cpu.compile() is ran and step._forward_kernel() is ran
    step.set_adjoint_pdfs(g)
    step.run_backward(2)
    ref, gref = TL._oracle_grad(f0, 1.3, 2, 'D2Q9', True, g)
    assert np.abs(np.asarray(step.pdf_array) - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(np.asarray(step.adjoint_pdf_array) - gref).max() <= 1e-12 * np.abs(gref).max()


def test_lattice_source_refusals():
    st = lbm.LBStencil('D2Q9')
    with pytest.raises(NotImplementedError, match='smagorinsky'):
        LatticeSource(st, True, 'float', False, smagorinsky=0.2, half=True)
    with pytest.raises(NotImplementedError, match='smagorinsky'):
        LatticeSource(st, True, 'double', False, smagorinsky=0.2, force_field=True, force_model='guo')


# --- 7. the sources --------------------------------------------------------------------------------------------
_SOURCE_KERNELS = {}


def _source_kernels(stencil, shape, field):
    """The HIP ``LatticeKernels`` of a walled family with link programs (a FixedDensity channel), made once."""
    key = (stencil, shape, field)
    if key not in _SOURCE_KERNELS:
        K = _step(stencil, shape, True, 'gpu', 'float32', field=field, walls='pressure')[0]._lattice_kernels()
        assert K.omega_field == field and K.programs is not None
        _SOURCE_KERNELS[key] = K
    return _SOURCE_KERNELS[key]


@pytest.mark.parametrize('fix', [False, True])
@pytest.mark.parametrize('addr', ['buf', 'ptr'])
@pytest.mark.parametrize('idx', ['int', 'long long'])
@pytest.mark.parametrize('field', [False, True])
@pytest.mark.parametrize('stencil,shape', [('D2Q9', (9, 8)), ('D3Q27', (6, 8, 5))])
def test_smagorinsky_sources_compile(monkeypatch, stencil, shape, field, idx, addr, fix):
    """(``int`` / ``long long``) × (``buf`` / ``ptr``) × (main / fix-up), with and without the ω field, compile to
    gfx950 code objects (one module per case); every source has exactly one definition of the effective rate, called
    once by the forward and once by the adjoint cell."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from tests.test_native_abi import _is_amdgpu_elf
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    src = _source_kernels(stencil, shape, field).source(idx, addr, fix=fix)
    assert src.count('float lbm_omega_eff(const float omega_0') == 1
    assert src.count('const float omega = lbm_omega_eff(') == 2
    assert src.count('const float omega =') == 2
    assert src.count('domega[wc] +=') == int(field)
    code = rt.compile_hip(src, name='psad_lbm.hip')
    assert _is_amdgpu_elf(code)
    for nm in (['lbm_adj_fix'] if fix else ['lbm_fwd', 'lbm_adj']):
        assert nm.encode() in code


@pytest.mark.parametrize('field', [False, True])
def test_smagorinsky_source_variants_differ(field):
    K = _source_kernels('D2Q9', (9, 8), field)
    assert len({K.source(idx, addr, fix=fix) for idx in ('int', 'long long') for addr in ('buf', 'ptr')
                for fix in (False, True)}) == 8


def test_smagorinsky_c_source_builds():
    for field in (False, True):
        Kc = _step('D2Q9', (9, 8), True, 'cpu', 'float32', field=field, walls='pressure')[0]._lattice_kernels()
        assert Kc.build() is not None


def _golden_module():
    spec = importlib.util.spec_from_file_location('make_lattice_smagorinsky_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_lattice_smagorinsky_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_smagorinsky_sources_pinned():
    """Every emitted source of the Smagorinsky variants (``make_lattice_smagorinsky_golden``) is the pinned one, and
    C_s is part of the source (so of every cache key made from it)."""
    mod = _golden_module()
    with open(os.path.join(GOLDEN_DIR, 'lattice_smagorinsky_source_sha.json')) as fh:
        golden = json.load(fh)
    shas = mod.shas()
    assert sorted(shas) == sorted(golden)
    assert [k for k in golden if shas[k] != golden[k]] == []
    a = mod.kernels('D2Q9-srt-periodic', 'float32', 'gpu').source()
    b = mod.kernels('D2Q9-srt-periodic', 'float32', 'gpu', cs=0.1).source()
    assert hashlib.sha256(a.encode()).hexdigest() != hashlib.sha256(b.encode()).hexdigest()


# --- GPU -------------------------------------------------------------------------------------------------------
#          stencil, shape, compressible, method, force model, layout, walls, ω field
GPU_F64 = [('D2Q9', (37, 70), True, 'srt', None, 'numpy', 'channel', False),
           ('D3Q19', (16, 12, 24), True, 'srt', None, 'fzyx', None, False),
           ('D3Q27', (10, 9, 66), True, 'srt', None, 'fzyx', 'channel', False),
           ('D2Q9', (37, 70), True, 'trt-magic', None, 'fzyx', 'channel', False),
           ('D2Q9', (37, 70), True, 'mrt', None, 'fzyx', 'channel', False),
           ('D2Q9', (37, 70), True, 'srt', 'guo', 'fzyx', None, False),
           ('D2Q9', (37, 70), True, 'srt', None, 'fzyx', None, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape,compressible,method,fm,layout,walls,field', GPU_F64)
def test_smagorinsky_lattice_gpu_vs_reference(stencil, shape, compressible, method, fm, layout, walls, field):
    """The HIP lattice kernels in float64, T = 3, at 1e-12 (pdfs) and 1e-11 (adjoints)."""
    res = _case(stencil, shape, compressible, 'gpu', method=method, fm=fm, layout=layout, walls=walls, field=field)
    _check(res, 1e-12, 1e-11)
    assert ('gW' in res) == field


@pytest.mark.gpu
def test_smagorinsky_fixup_launch_gpu():
    """Link-program walls (the pressure channel): the listed cells' adjoint comes from the fix-up launch, which shares
    the cell function; a second backward is bitwise equal to the first."""
    import torch
    shape = (70, 33)
    res = _case('D2Q9', shape, True, 'gpu', walls='pressure')
    _check(res, 1e-12, 1e-11)
    step = res['step']
    cells = step._cells_arg()
    assert cells is not None and int(cells.numel()) > 0
    x, _, gt = res['inputs']
    again = []
    for _ in range(2):
        x.grad = None
        step.create_timestep_op(3).apply(x).backward(gt)
        again.append(x.grad.clone())
    assert torch.equal(again[0], again[1]) and torch.equal(again[0].double().cpu(), res['gx'][0])


@pytest.mark.gpu
def test_smagorinsky_ptr_addressing_bitwise_gpu(monkeypatch):
    """``PSAD_LBM_ADDR=ptr``: bitwise equal to ``buf`` in float64."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    a = _case('D2Q9', (37, 70), True, 'gpu', layout='numpy', walls='channel')
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    b = _case('D2Q9', (37, 70), True, 'gpu', layout='numpy', walls='channel')
    assert {k[2] for k in b['step']._lattice_kernels()._fns} == {'ptr'}
    assert {k[2] for k in a['step']._lattice_kernels()._fns} == {'buf'}
    for k in ('out', 'gx'):
        assert torch.equal(a[k][0], b[k][0]), k


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape', [('D2Q9', (64, 48)), ('D3Q19', (20, 17, 70))])
def test_smagorinsky_float32_gpu(stencil, shape):
    """float32, no-slip channel with an obstacle, T = 3: the error of the pdfs and of the pdf adjoint against the
    float64 reference is at most 4× the error of the same reference run in float32 on the CPU on the same inputs
    (convention (b) of ``test_omega_field_float32_gpu``). Measured on an MI355X: ratios 0.87 – 1.50
    ("Smagorinsky")."""
    import torch
    res = _case(stencil, shape, True, 'gpu', 'float32', walls='channel')
    x, _, gt = res['inputs']
    wall = torch.tensor(res['walls'][1])
    x32 = x.detach().cpu().requires_grad_()
    ref32 = _reference(x32, OMEGA, 3, stencil, True, walls=('noslip', wall))
    (g32,) = torch.autograd.grad(ref32, x32, gt.cpu())
    for name, cpu32 in (('out', ref32.detach()), ('gx', g32)):
        got, ref = res[name]
        e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu32.double() - ref).abs().max())
        print(f'{stencil} {name}: error {e_gpu:.3e}, float32 reference {e_cpu:.3e}, ratio {e_gpu / e_cpu:.3f} (bound 4)')
    for name, cpu32 in (('out', ref32.detach()), ('gx', g32)):
        got, ref = res[name]
        assert float((got - ref).abs().max()) <= 4 * float((cpu32.double() - ref).abs().max()), name


@pytest.mark.gpu
def test_smagorinsky_schedules_agree_gpu():
    """The lattice kernels against the rule's AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``) on the same inputs."""
    a = _case('D2Q9', (37, 70), True, 'gpu', schedule='lattice')
    b = _case('D2Q9', (37, 70), True, 'gpu', schedule='autodiffop')
    _check(b, 1e-12, 1e-11)
    _check({k: (a[k][0], b[k][0]) for k in ('out', 'gx')}, 1e-12, 1e-11)
