"""A per-cell relaxation rate: ``create_lb_update_rule(relaxation_rate=w.center)`` with ``w`` a scalar field — an
additional input of the step whose adjoint ``dω(x) = Σ_t Σ_i g_i ∂dst_i/∂ω`` the adjoint kernels accumulate.

Reference: ``oracle/lbm.py``'s collision with ω a ``[*domain]`` tensor (``trt_odd_rate`` of it for TRT; MRT composed
from two constant matrices, ``_collide``) and torch's reverse mode through it. The lattice kernels (C and HIP) and the
rule's AutoDiffOp kernels (the generic transposed derivation) are each held against it, and against each other."""
import os

import numpy as np
import pytest
import sympy as sp

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from pystencils_autodiff_amd.lbm import _lattice_kernels as LK
from tests import test_lbm as TL
from tests import test_lbm_neighbour_links as TN
from tests.test_lbm import _channel, _init, _set_channel

FORCE = {2: (1e-3, -2e-3), 3: (1e-3, -2e-3, 1.5e-3)}
MRT_CONST = dict(bulk=1.1, third=1.3, fourth=1.2)            # relaxation_rates=[ω, 1.1, 1.3, 1.2]
ODD_RATE = 1.2                                               # the constant odd rate of TRT 'rate'


# --- the reference ---------------------------------------------------------------------------------------------
def _collide(fs, W, stencil, compressible, method, fm, force, xp):
    """The collision of streamed pdfs ``fs`` with the per-cell rate ``W`` (``[*domain]``)."""
    if method == 'mrt':
        # A = ω P_ω + C: dst = f − ω P_ω n − C n, from two constant-matrix collisions (no force)
        assert fm is None
        zero = dict(bulk=0.0, third=0.0, fourth=0.0)
        a = OL.collide(fs, None, stencil, compressible, xp, mrt=OL.mrt_matrix(stencil, dict(zero, shear=1.0)))
        b = OL.collide(fs, None, stencil, compressible, xp, mrt=OL.mrt_matrix(stencil, dict(MRT_CONST, shear=0.0)))
        return fs + W[..., None] * (a - fs) + (b - fs)
    odd = OL.trt_odd_rate(W) if method == 'trt-magic' else ODD_RATE if method == 'trt-rate' else None
    return OL.collide(fs, W, stencil, compressible, xp, fm, force, odd)


def _reference(f, W, T, stencil, compressible, method='srt', fm=None, force=None, walls=None):
    """``T`` steps in torch. ``walls``: None, ``('noslip', wall)``, ``('pressure', wall, pressure, rho_w)`` or
    ``('links', ids, kinds)`` (the restatement of ``test_lbm_neighbour_links``)."""
    import torch
    for _ in range(T):
        if walls is None:
            fs, keep = OL.stream(f, stencil, torch), None
        elif walls[0] == 'noslip':
            fs, keep = OL.stream_walls(f, stencil, walls[1], torch), walls[1]
        elif walls[0] == 'pressure':
            fs, keep = OL.stream_pressure_walls(f, stencil, walls[1], walls[2], walls[3], compressible, torch), walls[1]
        else:
            fs, keep = TN.stream_links(f, stencil, walls[1], walls[2], compressible, torch), walls[1] != 0
        new = _collide(fs, W, stencil, compressible, method, fm, force, torch)
        f = new if keep is None else torch.where(keep.unsqueeze(-1), f, new)
    return f


# --- the step --------------------------------------------------------------------------------------------------
def _schedule_env(schedule):
    class _Env:
        def __enter__(self):
            self.old = os.environ.get('PSAD_LBM_LATTICE')
            os.environ['PSAD_LBM_LATTICE'] = '1' if schedule == 'lattice' else '0'

        def __exit__(self, *a):
            if self.old is None:
                os.environ.pop('PSAD_LBM_LATTICE')
            else:
                os.environ['PSAD_LBM_LATTICE'] = self.old
    return _Env()


def _rule(stencil, compressible, dtype='float64', method='srt', fm=None, force=None, layout='fzyx', name='omega_f'):
    D = lbm.LBStencil(stencil).D
    w = ps.fields(f'{name}: {dtype}[{D}D]')
    kw = {}
    if method == 'trt-magic':
        kw = dict(method='trt')
    elif method == 'trt-rate':
        kw = dict(method='trt', relaxation_rates=[w.center, ODD_RATE])
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[w.center, MRT_CONST['bulk'], MRT_CONST['third'], MRT_CONST['fourth']])
    if 'relaxation_rates' not in kw:
        kw['relaxation_rate'] = w.center
    if fm is not None:
        kw.update(force_model=fm, force=force)
    return lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, layout=layout, **kw), w


def _step(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, force=None, layout='fzyx',
          schedule='lattice', walls=None):
    """(step, reference walls) — the step needs no ``relaxation_rate``: the rule's only scalar is the field."""
    rule, w = _rule(stencil, compressible, dtype, method, fm, force, layout)
    with _schedule_env(schedule):
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target=target)
    assert (step._lattice is not None) == (schedule == 'lattice')
    assert w in step._additional_fields
    D = len(shape)
    ref_walls = None
    if walls == 'channel':
        _set_channel(step, shape)
        ref_walls = ('noslip', _channel(shape))
    elif walls == 'pressure':
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
        ref_walls = ('pressure', wall | pressure, pressure, rho_w)
        assert step._lattice_kernels().programs is not None
    elif walls == 'slip':
        kinds = {}
        for end, sign in ((0, 1), (-1, -1)):
            n = TN._unit(D, 1, sign)
            bc = lbm.FreeSlip(n)
            step.set_boundary_including_adjoint(bc, TN._end(D, 1, end))
            kinds[step.boundary_handling.conditions[bc]] = ('freeslip', n)
        ref_walls = ('links', step.boundary_handling.flags.astype(np.int64), kinds)
        assert step._lattice_kernels().programs is not None
    if ref_walls is not None:
        assert np.array_equal(step.boundary_handling.flags != 0,
                              ref_walls[1] if ref_walls[0] != 'links' else ref_walls[1] != 0)
    return step, ref_walls


def _inputs(stencil, shape, compressible, seed, force_field=False):
    rng = np.random.default_rng(seed)
    f0 = _init(stencil, shape, compressible, seed=seed + 1)
    W = rng.uniform(0.6, 1.9, shape)
    g = rng.standard_normal(f0.shape)
    Fv = 1e-3 * rng.standard_normal(shape + (len(shape),)) if force_field else None
    return f0, W, g, Fv


def _case(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, force_kind=None, layout='fzyx',
          schedule='lattice', walls=None, T=3, seed=11):
    """The timestep op against the reference: dict of (got, reference) pairs for the pdfs ``out``, the pdf adjoint
    ``gx``, the ω adjoint ``gW`` (and the force adjoint ``gF``), as float64 CPU tensors, plus the step."""
    import torch
    D = len(shape)
    F = ps.fields(f'F({D}): {dtype}[{D}D]') if force_kind == 'field' else None
    force = F if F is not None else FORCE[D] if fm is not None else None
    step, ref_walls = _step(stencil, shape, compressible, target, dtype, method, fm, force, layout, schedule, walls)
    extras = [f.name for f in step._additional_fields]
    assert extras == (['F', 'omega_f'] if F is not None else ['omega_f'])          # sorted by name
    op = step.create_timestep_op(T)
    f0, W, g, Fv = _inputs(stencil, shape, compressible, seed, F is not None)
    dev = 'cuda' if target == 'gpu' else 'cpu'
    tdt = getattr(torch, dtype)
    # (the reference runs on the inputs as the kernels see them: rounded to the pdf dtype)
    x, Wt = (torch.tensor(a, dtype=tdt, device=dev, requires_grad=True) for a in (f0, W))
    Ft = torch.tensor(Fv, dtype=tdt, device=dev, requires_grad=True) if F is not None else None
    gt = torch.tensor(g, dtype=tdt, device=dev)
    out = op.apply(x, *([Ft, Wt] if F is not None else [Wt]))
    out.backward(gt)
    xr, Wr = x.detach().double().cpu().requires_grad_(), Wt.detach().double().cpu().requires_grad_()
    Fr = Ft.detach().double().cpu().requires_grad_() if F is not None else None
    rw = None if ref_walls is None else (ref_walls[0],) + tuple(
        torch.tensor(a) if isinstance(a, np.ndarray) else a for a in ref_walls[1:])
    rforce = tuple(Fr[..., a] for a in range(D)) if F is not None else force
    ref = _reference(xr, Wr, T, stencil, compressible, method, fm, rforce, rw)
    grads = torch.autograd.grad(ref, (xr, Wr) + ((Fr,) if F is not None else ()), gt.double().cpu())
    res = dict(out=(out.detach().double().cpu(), ref.detach()), gx=(x.grad.double().cpu(), grads[0]),
               gW=(Wt.grad.double().cpu(), grads[1]))
    if F is not None:
        res['gF'] = (Ft.grad.double().cpu(), grads[2])
    res['step'], res['walls'], res['inputs'] = step, ref_walls, (x, Wt, gt, Ft)
    return res


def _check(res, tol, gtol):
    for name, t in (('out', tol), ('gx', gtol), ('gW', gtol), ('gF', gtol)):
        if name in res:
            got, ref = res[name]
            err, scale = float((got - ref).abs().max()), float(ref.abs().max())
            print(f'{name}: max error {err:.3e} of max {scale:.3e} (ratio {err / scale:.3e}, bound {t:.0e})')
            assert scale > 0 and err <= t * scale, (name, err, scale)


# --- CPU: the lattice schedule ---------------------------------------------------------------------------------
#             stencil, shape, compressible, method, force model, force kind, layout, walls
CPU_LATTICE = [('D2Q9', (9, 7), True, 'srt', None, None, 'fzyx', None),
               ('D2Q9', (9, 7), False, 'srt', None, None, 'fzyx', None),
               ('D2Q9', (12, 9), True, 'srt', None, None, 'fzyx', 'channel'),
               ('D3Q19', (5, 4, 6), True, 'srt', None, None, 'fzyx', None),
               ('D2Q9', (9, 7), True, 'trt-magic', None, None, 'fzyx', None),
               ('D2Q9', (9, 7), False, 'trt-rate', None, None, 'fzyx', None),
               ('D2Q9', (9, 7), True, 'mrt', None, None, 'fzyx', None),
               ('D3Q19', (5, 4, 6), False, 'mrt', None, None, 'fzyx', None),
               ('D2Q9', (9, 7), True, 'srt', 'guo', 'const', 'fzyx', None),
               ('D2Q9', (9, 7), False, 'srt', 'simple', 'const', 'fzyx', None),
               ('D2Q9', (9, 7), True, 'srt', 'guo', 'field', 'fzyx', None),
               ('D2Q9', (9, 7), True, 'trt-magic', 'guo', 'field', 'fzyx', None),
               ('D2Q9', (9, 7), True, 'srt', None, None, 'numpy', None)]


@pytest.mark.parametrize('stencil,shape,compressible,method,fm,force_kind,layout,walls', CPU_LATTICE)
def test_omega_field_lattice_cpu_vs_oracle(stencil, shape, compressible, method, fm, force_kind, layout, walls):
    """The C lattice kernels, float64, T = 3 through the timestep op: pdfs, pdf adjoint, ``dω`` (and ``dF``, returned
    in the order of the extras) against the oracle at the tolerances of ``test_lbm_force_field_cpu_vs_oracle``;
    wall cells get exactly 0."""
    res = _case(stencil, shape, compressible, 'cpu', method=method, fm=fm, force_kind=force_kind, layout=layout,
                walls=walls)
    assert res['step']._lattice_kernels().omega_field
    _check(res, 1e-13, 1e-12)
    if walls:
        wall = res['walls'][1]
        assert wall.any() and float(res['gW'][1][wall].abs().max()) == 0.0
        assert float(res['gW'][0][wall].abs().max()) == 0.0
        assert float(res['gW'][0][~wall].abs().min()) > 0.0


# --- CPU: the AutoDiffOp schedule ------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['srt', 'trt-magic'])
def test_omega_field_autodiffop_cpu_vs_oracle(method):
    """``PSAD_LBM_LATTICE=0``: the plain ω field on the rule's AutoDiffOp kernels (the generic transposed derivation,
    an implementation independent of the lattice kernels' ``omega_adjoint``)."""
    res = _case('D2Q9', (8, 6), True, 'cpu', method=method, schedule='autodiffop')
    _check(res, 1e-13, 1e-12)


def test_omega_from_viscosity_field_cpu():
    """ω = 1/(3 ν(x) + ½): not a plain field read, so the rule's AutoDiffOp kernels run it and return dν."""
    import torch
    shape, T = (8, 6), 3
    nu = ps.fields('nu: float64[2D]')
    rule = lbm.create_lb_update_rule('D2Q9', relaxation_rate=1 / (3 * nu.center + sp.Rational(1, 2)), compressible=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu')
    assert step._lattice is None and step._additional_fields == [nu]
    f0, W, g, _ = _inputs('D2Q9', shape, True, 21)
    nu0 = (1 / W - 0.5) / 3
    x, nt = torch.tensor(f0, requires_grad=True), torch.tensor(nu0, requires_grad=True)
    out = step.create_timestep_op(T).apply(x, nt)
    out.backward(torch.tensor(g))
    xr, nr = torch.tensor(f0, requires_grad=True), torch.tensor(nu0, requires_grad=True)
    ref = _reference(xr, 1 / (3 * nr + 0.5), T, 'D2Q9', True)
    gx, gn = torch.autograd.grad(ref, (xr, nr), torch.tensor(g))
    _check(dict(out=(out.detach(), ref.detach()), gx=(x.grad, gx), gW=(nt.grad, gn)), 1e-13, 1e-12)


@pytest.mark.parametrize('what', ['offset', 'dtype'])
def test_other_omega_expressions_take_the_autodiffop_schedule(what):
    """A rate read at an offset, or from a field of another dtype, is not the lattice kernels' case."""
    w = ps.fields('w: float64[2D]') if what == 'offset' else ps.fields('w: float32[2D]')
    rule = lbm.create_lb_update_rule('D2Q9', relaxation_rate=w[1, 0] if what == 'offset' else w.center)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(6, 5), target='cpu')
    assert step._lattice is None and step._omega_field is None and step._additional_fields == [w]


# --- the dω formulas against the symbolic rule -----------------------------------------------------------------
@pytest.mark.parametrize('guo', [False, True])
@pytest.mark.parametrize('method', ['srt', 'trt-magic', 'trt-rate', 'mrt'])
def test_domega_formulas_match_the_symbolic_rule(method, guo):
    """``∂dst_i/∂ω`` by ``sp.diff`` of the D2Q9 rule (subexpressions inlined) against the formulas of
    ``_lattice_source.omega.omega_adjoint``: SRT ``−n_i``; TRT ``−(a′ n_i + b′ n_ī)``; MRT ``−(P_ω n)_i``; Guo adds
    ``−½ w_i T_i`` — evaluated at a random state (exact rationals)."""
    from pystencils_autodiff_amd.lbm._method import mrt_relaxation_matrices
    st = lbm.LBStencil('D2Q9')
    Fc = (sp.Rational(1, 700), sp.Rational(-1, 300))
    rule, w = _rule('D2Q9', True, method=method, fm='guo' if guo else None, force=Fc if guo else None)
    om = w.center
    flat = rule.new_without_subexpressions()
    rng = np.random.default_rng(5)
    acc = sorted(flat.atoms(ps.Field.Access) - {om} - {a.lhs for a in flat.main_assignments}, key=str)
    assert len(acc) == 9
    vals = {a: sp.Rational(int(rng.integers(50, 150)), 900) for a in acc}
    vals[om] = sp.Rational(13, 10)
    f = [next(a for a in acc if tuple(a.index) == (i,)) for i in range(9)]          # the pulled pdfs src_i(x − c_i)
    assert all(tuple(int(o) for o in f[i].offsets) == tuple(-c for c in st.directions[i]) for i in range(9))
    rho = sum(f)
    u = [(sum(c[a] * fi for c, fi in zip(st.directions, f)) + (Fc[a] / 2 if guo else 0)) / rho for a in range(2)]
    usq = sum(ua ** 2 for ua in u)
    n, T = [], []
    for i, c in enumerate(st.directions):
        cu = sum(ca * ua for ca, ua in zip(c, u))
        n.append(f[i] - st.weights[i] * rho * (1 + 3 * cu + sp.Rational(9, 2) * cu ** 2 - sp.Rational(3, 2) * usq))
        cF = sum(ca * Fa for ca, Fa in zip(c, Fc))
        T.append(3 * sum((ca - ua) * Fa for ca, ua, Fa in zip(c, u, Fc)) + 9 * cu * cF)
    inv = [st.inverse_direction_index(i) for i in range(9)]
    if method == 'trt-magic':
        lam = sp.Rational(3, 16)
        wp = -16 * lam / (4 * lam * om + 2 - om) ** 2
    else:
        wp = 0
    Pw = mrt_relaxation_matrices(st)['shear']
    size = []
    for i, asg in enumerate(flat.main_assignments):
        got = sp.diff(asg.rhs, om).subs(vals)
        if method == 'srt':
            want = -n[i]
        elif method == 'mrt':
            want = -sum(Pw[i][k] * n[k] for k in range(9))
        else:
            want = -((1 + wp) / 2 * n[i] + (1 - wp) / 2 * n[inv[i]])
        if guo:
            want = want - st.weights[i] * T[i] / 2
        want = sp.sympify(want).subs(vals)
        # (the constant rates of TRT 'rate' / MRT are floats in the rule: equal to rounding, exact otherwise)
        assert abs(sp.N(got - want, 30)) <= 1e-13, (method, guo, i, got, want)
        size.append(abs(float(want)))
    assert min(size[1:]) > 1e-4                    # (MRT: the shear projector's row of the rest population is 0)


# --- the public interface --------------------------------------------------------------------------------------
def test_scalar_rate_through_expand():
    """A trainable scalar rate: ``w0.expand(*domain)`` as the field tensor, ``w0.grad = Σ_x dω(x)`` by torch's own
    reduction of the expanded tensor's gradient."""
    import torch
    shape, T = (9, 7), 3
    step, _ = _step('D2Q9', shape, True, 'cpu')
    op = step.create_timestep_op(T)
    f0, _, g, _ = _inputs('D2Q9', shape, True, 31)
    w0 = torch.tensor(1.37, dtype=torch.float64, requires_grad=True)
    op.apply(torch.tensor(f0), w0.expand(*shape)).backward(torch.tensor(g))
    Wf = torch.full(shape, 1.37, dtype=torch.float64, requires_grad=True)
    op.apply(torch.tensor(f0), Wf).backward(torch.tensor(g))
    total = float(Wf.grad.sum())
    assert w0.grad.shape == () and abs(float(w0.grad) - total) <= 1e-12 * abs(total)
    # ... and it is the derivative of the scalar-ω step
    wr = torch.tensor(1.37, dtype=torch.float64, requires_grad=True)
    ref = OL.run(torch.tensor(f0), wr, T, 'D2Q9', True, xp=torch)
    (gw,) = torch.autograd.grad(ref, wr, torch.tensor(g))
    assert abs(float(w0.grad) - float(gw)) <= 1e-12 * abs(float(gw))


def test_omega_field_end_to_end_op():
    """``create_end_to_end_op(additional_fields_to_tensor_map={w: W})``: the tensor reaches every step; dloss/dω at
    three cells against central differences (the bound of ``test_lbm_force_field_end_to_end_and_errors``)."""
    import torch
    shape = (9, 7)
    rule, w = _rule('D2Q9', True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu')
    rng = np.random.default_rng(1)
    rho = torch.tensor(1 + 0.01 * rng.standard_normal(shape))
    vel = torch.tensor(0.03 * rng.standard_normal(shape + (2,)))
    Wt = torch.tensor(rng.uniform(0.6, 1.9, shape), requires_grad=True)

    def loss(Wv):
        r = step.create_end_to_end_op(4, vel, rho, additional_fields_to_tensor_map={w: Wv},
                                      num_times_steps_without_save=1)
        # (a loss of O(0.1): its rounding noise in the difference quotient, ε·|loss|/e, stays below the bound's 1e-9)
        return (r.output_velocity_tensor ** 2).sum() + ((r.output_density_tensor - 1) ** 2).sum()
    loss(Wt).backward()
    e = 1e-6
    for idx in ((3, 2), (0, 6), (8, 0)):
        Wp, Wm = Wt.detach().clone(), Wt.detach().clone()
        Wp[idx] += e
        Wm[idx] -= e
        fd = (float(loss(Wp)) - float(loss(Wm))) / (2 * e)
        assert abs(fd - float(Wt.grad[idx])) <= 1e-6 * abs(fd) + 1e-9, (idx, fd, float(Wt.grad[idx]))
    with pytest.raises(ValueError, match='omega_f'):
        step.create_end_to_end_op(4, vel, rho)


def test_omega_field_run_and_run_backward():
    """``run`` / ``run_backward(extra=…, extra_adj=…)`` take the field and its adjoint array like the force's."""
    import torch
    shape, T = (9, 7), 3
    step, _ = _step('D2Q9', shape, True, 'cpu')
    f0, W, g, _ = _inputs('D2Q9', shape, True, 41)
    step.set_pdfs(f0)
    step.run(T, record=True, extra={'omega_f': W})
    dW = np.zeros_like(W)
    step.set_adjoint_pdfs(g)
    step.run_backward(T, extra={'omega_f': W}, extra_adj={'diffomega_f': dW})
    xr, Wr = torch.tensor(f0, requires_grad=True), torch.tensor(W, requires_grad=True)
    ref = _reference(xr, Wr, T, 'D2Q9', True)
    gx, gW = torch.autograd.grad(ref, (xr, Wr), torch.tensor(g))
    _check(dict(out=(torch.tensor(step.pdf_array), ref.detach()), gx=(torch.tensor(step.adjoint_pdf_array), gx),
                gW=(torch.tensor(dW), gW)), 1e-13, 1e-12)


def test_omega_field_errors():
    """Wrong shape, wrong dtype, missing tensor, missing adjoint array, a field with an index dimension."""
    import torch
    shape = (9, 7)
    step, _ = _step('D2Q9', shape, True, 'cpu')
    op = step.create_timestep_op(2)
    f0, W, g, _ = _inputs('D2Q9', shape, True, 51)
    x = torch.tensor(f0)
    with pytest.raises(ValueError, match='shape'):
        op.apply(x, torch.tensor(W[:-1]))
    with pytest.raises(ValueError, match='dtype'):
        op.apply(x, torch.tensor(W, dtype=torch.float32))
    with pytest.raises(TypeError, match='omega_f'):
        op.apply(x)
    step.set_pdfs(f0)
    with pytest.raises(ValueError, match='omega_f'):
        step.run(1)
    step.run(1, record=True, extra={'omega_f': W})
    with pytest.raises(ValueError, match='diffomega_f'):
        step.run_backward(1, extra={'omega_f': W})
    with pytest.raises(ValueError, match='strides'):
        step.run_backward(1, extra={'omega_f': W}, extra_adj={'diffomega_f': np.zeros(shape[::-1]).T})
    wv = ps.fields('wv(2): float64[2D]')
    with pytest.raises(ValueError, match='wv'):
        lbm.AutoDiffLatticeBoltzmannStep(lbm.create_lb_update_rule('D2Q9', relaxation_rate=wv.center(0)),
                                         domain_size=shape, target='cpu')
    # kernels without the field refuse one; LatticeKernels keeps its positional parameters (omega_field: keyword only)
    K = LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float64, False, 'cpu')
    src, dst = np.ascontiguousarray(f0), np.empty_like(f0)
    with pytest.raises(ValueError, match='no relaxation-rate field'):
        K.forward(src, dst, 1.0, omf=W)
    with pytest.raises(TypeError):
        LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float64, False, 'cpu', None, None, None, False, None, None,
                          None, True)


# --- the sources -----------------------------------------------------------------------------------------------
def test_omega_field_sources_compile(monkeypatch):
    """The ω-field variants of one walled family with link programs (a FixedDensity channel): (``int`` / ``long
    long``) × (``buf`` / ``ptr``) × (main / fix-up) compile to gfx950 code objects, the C twin with gcc, and the
    argument buffer of ``plan()`` has the kernel signature's pointers and strides."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from tests.test_native_abi import _is_amdgpu_elf
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    K = _step('D2Q9', (9, 8), True, 'gpu', 'float32', walls='pressure')[0]._lattice_kernels()
    assert K.omega_field and K.programs is not None
    sources = set()
    for idx in ('int', 'long long'):
        for addr in ('buf', 'ptr'):
            for fix in (False, True):
                src = K.source(idx, addr, fix=fix)
                assert 'const float omega = (float)omf[wc];' in src and 'domega[wc] += (T)dom;' in src
                assert src.count('domega[wc] +=') == 1
                sources.add(src)
                code = rt.compile_hip(src, name='psad_lbm.hip')
                assert _is_amdgpu_elf(code)
                for nm in (['lbm_adj_fix'] if fix else ['lbm_fwd', 'lbm_adj']):
                    assert nm.encode() in code
                # pointers: 3 pdf arrays, mask, ids, omf, domega; strides: 3 × 4 + 3
                sig = src[src.index('lbm_adj_fix(' if fix else 'lbm_adj('):]
                sig = sig[:sig.index(')')]
                assert sig.count('*') == 7 + int(fix) and sig.count('const IDX') == 15
    assert len(sources) == 8
    Kc = _step('D2Q9', (9, 8), True, 'cpu', 'float32', walls='pressure')[0]._lattice_kernels()
    assert Kc.build() is not None
    # a field that reaches 2³¹ − 1 elements widens the index type alone
    import torch
    pdfs = [torch.empty((6, 5, 9), dtype=torch.float32, device='meta')] * 3
    far = torch.empty_strided((6, 5), (2 ** 31 // 5, 1), dtype=torch.float32, device='meta')
    near = torch.empty((6, 5), dtype=torch.float32, device='meta')
    assert K._launch_mode(pdfs, {'omega': (near, near)}) == ('int', 'buf')
    assert K._launch_mode(pdfs, {'omega': (far, far)}) == ('long long', 'buf')


# --- GPU -------------------------------------------------------------------------------------------------------
#          stencil, shape, compressible, method, force model, force kind, layout, walls
GPU_F64 = [('D2Q9', (37, 70), False, 'srt', None, None, 'numpy', 'channel'),
           ('D3Q19', (16, 12, 24), True, 'srt', None, None, 'fzyx', None),
           ('D3Q27', (10, 9, 66), True, 'srt', None, None, 'fzyx', 'channel'),
           ('D2Q9', (37, 70), True, 'trt-magic', None, None, 'fzyx', 'channel'),
           ('D2Q9', (37, 70), True, 'mrt', None, None, 'fzyx', 'channel'),
           ('D3Q19', (20, 17, 70), True, 'srt', 'guo', 'field', 'fzyx', None)]


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape,compressible,method,fm,force_kind,layout,walls', GPU_F64)
def test_omega_field_lattice_gpu_vs_oracle(stencil, shape, compressible, method, fm, force_kind, layout, walls):
    """The HIP lattice kernels in float64 at the existing GPU tolerances (1e-12 forward, 1e-11 adjoints)."""
    res = _case(stencil, shape, compressible, 'gpu', method=method, fm=fm, force_kind=force_kind, layout=layout,
                walls=walls)
    _check(res, 1e-12, 1e-11)
    if walls:
        assert float(res['gW'][0][res['walls'][1]].abs().max()) == 0.0


@pytest.mark.gpu
def test_omega_field_schedules_agree_gpu():
    """The lattice kernels against the rule's AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``) on the same inputs."""
    a = _case('D2Q9', (37, 70), True, 'gpu', schedule='lattice')
    b = _case('D2Q9', (37, 70), True, 'gpu', schedule='autodiffop')
    _check(b, 1e-12, 1e-11)
    _check({k: (a[k][0], b[k][0]) for k in ('out', 'gx', 'gW')}, 1e-12, 1e-11)


@pytest.mark.gpu
@pytest.mark.parametrize('walls,shape', [('pressure', (70, 33)), ('slip', (70, 33))])
def test_omega_field_fixup_launch_gpu(walls, shape):
    """Link-program walls: the listed cells' ``dω`` comes from the fix-up launch, and only from it — equal to the
    oracle's there; on these flat walls a second backward gives bitwise the same ``dω``."""
    import torch
    res = _case('D2Q9', shape, True, 'gpu', walls=walls)
    _check(res, 1e-12, 1e-11)
    step = res['step']
    cells = step._cells_arg()
    assert cells is not None and int(cells.numel()) > 0
    listed = np.zeros(int(np.prod(shape)), bool)
    listed[cells.cpu().numpy()] = True
    listed = torch.tensor(listed.reshape(shape))
    got, ref = res['gW']
    assert float(ref[listed].abs().min()) > 0
    assert float((got[listed] - ref[listed]).abs().max()) <= 1e-11 * float(ref.abs().max())
    x, Wt, gt, _ = res['inputs']
    again = []
    for _ in range(2):
        x.grad = Wt.grad = None
        step.create_timestep_op(3).apply(x, Wt).backward(gt)
        again.append(Wt.grad.clone())
    assert torch.equal(again[0], again[1]) and torch.equal(again[0].double().cpu(), got)


@pytest.mark.gpu
def test_omega_field_ptr_addressing_bitwise_gpu(monkeypatch):
    """``PSAD_LBM_ADDR=ptr``: bitwise equal to ``buf`` in float64."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    a = _case('D2Q9', (37, 70), False, 'gpu', layout='numpy', walls='channel')
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    b = _case('D2Q9', (37, 70), False, 'gpu', layout='numpy', walls='channel')
    assert {k[2] for k in b['step']._lattice_kernels()._fns} == {'ptr'}
    assert {k[2] for k in a['step']._lattice_kernels()._fns} == {'buf'}
    for k in ('out', 'gx', 'gW'):
        assert torch.equal(a[k][0], b[k][0]), k


def _chain_length(Q):
    """k of bound (a): the longest dependent fp32 chain from loaded values to ``dω`` in the emitted adjoint cell
    (SRT, compressible — the incompressible one is shorter; ``dom = −Σ g_k f_k`` first, a chain of Q + 1, then
    ``dom += g_k feq_k``): ρ = f0 + … (Q − 1 adds), 1/ρ and u_a = m_a/ρ (2), c·u (1: at most two nonzero axes on
    D2Q9 / D3Q19), poly = cu (3 + 4.5 cu) − 1.5 u² (4), feq = (w ρ)(1 + poly) (2), g · feq (1), and the Q sequential
    ``dom += …`` — 2 Q + 9. (The store ``domega += dom`` onto the zeroed array is exact at T = 1.)"""
    return 2 * Q + 9


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape,compressible,layout', [('D2Q9', (64, 48), True, 'fzyx'),
                                                              ('D3Q19', (20, 17, 70), False, 'fzyx')])
def test_omega_field_float32_gpu(stencil, shape, compressible, layout):
    """float32, no-slip channel with an obstacle: pdfs and the pdf adjoint at the tolerances of
    ``test_lbm_lattice_schedule_gpu_vs_oracle`` (1e-5, 1e-4 of the maximum). ``dω`` is a cancelling sum, so:
    (a) T = 1, per cell: ``|dω − ref| ≤ k 2⁻²⁴ Σ_i |g_i| (|f_i| + |feq_i|)`` (float64 oracle), k = ``_chain_length``;
    (b) T = 3: the error against the float64 oracle is at most 4× the error of the same oracle run in float32 on the
    CPU on the same inputs.
    Measured on an MI355X (worst ratio got / bound): see DESIGN.md, "ω field"."""
    import torch
    Q = len(OL.SETS[stencil][0])
    # (a)
    res = _case(stencil, shape, compressible, 'gpu', 'float32', layout=layout, walls='channel', T=1)
    x, Wt, gt, _ = res['inputs']
    wall = torch.tensor(res['walls'][1])
    fs = OL.stream_walls(x.detach().double().cpu(), stencil, wall, torch)
    rho = fs.sum(-1)
    dirs = OL.SETS[stencil][0]
    u = torch.stack([sum(c[a] * fs[..., i] for i, c in enumerate(dirs) if c[a]) / (rho if compressible else 1)
                     for a in range(len(shape))], -1)
    feq = OL.equilibrium(rho, u, stencil, compressible, xp=torch)
    bound = _chain_length(Q) * 2.0 ** -24 * (gt.double().cpu().abs() * (fs.abs() + feq.abs())).sum(-1)
    got, ref = res['gW']
    err = (got - ref).abs()
    fluid = ~wall
    print(f'(a) {stencil}: worst |dω − ref| / bound = {float((err[fluid] / bound[fluid]).max()):.3f} '
          f'(k = {_chain_length(Q)}); |dω| max {float(ref.abs().max()):.3e}')
    assert bool((err[fluid] <= bound[fluid]).all()) and float(got[wall].abs().max()) == 0.0
    # (b)
    res = _case(stencil, shape, compressible, 'gpu', 'float32', layout=layout, walls='channel', T=3)
    _check({k: res[k] for k in ('out', 'gx')}, 1e-5, 1e-4)
    x, Wt, gt, _ = res['inputs']
    x32, W32 = x.detach().cpu().requires_grad_(), Wt.detach().cpu().requires_grad_()
    ref32 = _reference(x32, W32, 3, stencil, compressible, walls=('noslip', wall))
    (g32,) = torch.autograd.grad(ref32, W32, gt.cpu())
    got, ref = res['gW']
    e_gpu, e_cpu = float((got - ref).abs().max()), float((g32.double() - ref).abs().max())
    print(f'(b) {stencil}: error {e_gpu:.3e}, float32 oracle {e_cpu:.3e}, ratio {e_gpu / e_cpu:.3f} (bound 4)')
    assert e_gpu <= 4 * e_cpu
