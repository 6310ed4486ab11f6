"""A per-cell solid fraction (partial bounce-back, Walsh, Burwinkle and Saar): ``create_lb_update_rule(...,
solid_fraction=s.center)`` with ``s`` a scalar field — with ``f_i`` the pulled pdfs and ``c_i`` what the rule assigns
without the keyword,

    dst_i = (1 − σ) c_i + σ f_ī,

an additional input of the step whose adjoint ``dσ(x) = Σ_t Σ_i g_i (f_ī − c_i)`` the adjoint kernels accumulate.

Reference: ``oracle/lbm.py``'s streaming and collision (``test_lbm_omega_field._collide``; Smagorinsky's rate from
``test_lbm_smagorinsky._omega_eff``) blended HERE with the streamed pdfs of the opposite directions, in torch float64,
and torch's reverse mode through T steps. σ is uniform in (0.05, 0.95) with three fluid cells at exactly 0 and three at
exactly 1; every parity case asserts that both kinds are present and that the reference's ``max |dσ|`` is positive."""
import numpy as np
import pytest
import sympy as sp

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from pystencils_autodiff_amd.lbm import _lattice_kernels as LK
from pystencils_autodiff_amd.lbm._lattice_source import LatticeSource, kernel_args
from tests import test_lbm_macroscopic_outputs as TM
from tests import test_lbm_neighbour_links as TN
from tests import test_lbm_omega_field as TO
from tests import test_lbm_smagorinsky as TS
from tests.test_lbm import _init

OMEGA = 1.7
CS = TS.CS
FORCE = TO.FORCE


# --- the reference ---------------------------------------------------------------------------------------------
def _reference_states(f, S, W, T, stencil, compressible, method='srt', fm=None, force=None, walls=None, cs=None):
    """The states 1 … T in torch from state 0 ``f`` (plain pdfs), the solid fraction ``S`` and the rate ``W`` (both
    ``[*domain]``). ``walls`` as ``test_lbm_omega_field._reference``."""
    import torch
    inv = OL.inverse(stencil)
    states = []
    for _ in range(T):
        if walls is None:
            fs, keep = OL.stream(f, stencil, torch), None
        elif walls[0] == 'noslip':
            fs, keep = OL.stream_walls(f, stencil, walls[1], torch), walls[1]
        elif walls[0] == 'pressure':
            fs, keep = OL.stream_pressure_walls(f, stencil, walls[1], walls[2], walls[3], compressible, torch), walls[1]
        else:
            fs, keep = TN.stream_links(f, stencil, walls[1], walls[2], compressible, torch), walls[1] != 0
        Wc = W if cs is None else TS._omega_eff(fs, W, stencil, compressible, fm, force, cs)[0]
        c = TO._collide(fs, Wc, stencil, compressible, method, fm, force, torch)
        new = (1 - S)[..., None] * c + S[..., None] * fs[..., inv]
        f = new if keep is None else torch.where(keep.unsqueeze(-1), f, new)
        states.append(f)
    return states


# --- the step --------------------------------------------------------------------------------------------------
def _rule(stencil, compressible, dtype='float64', method='srt', fm=None, force=None, layout='fzyx', field=False,
          cs=None, zc=False, sigma='field'):
    """(rule, σ field, ω field); ``sigma``: 'field' (``s.center``), None (no keyword) or any value of the keyword."""
    D = lbm.LBStencil(stencil).D
    s = ps.fields(f'sigma: {dtype}[{D}D]')
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
    if sigma is not None:
        kw['solid_fraction'] = s.center if isinstance(sigma, str) and sigma == 'field' else sigma
    return lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, layout=layout,
                                     zero_centered=zc, smagorinsky=cs if cs is not None else False, **kw), s, w


def _set_walls(step, shape, walls):
    """'channel' (no-slip, with an obstacle), 'pressure' (FixedDensity inlet / outlet: link programs) or 'slip'
    (FreeSlip: neighbour links) on ``step``; returns the reference's description and the bool mask of wall cells."""
    D = len(shape)
    if walls in ('channel', 'pressure'):
        ref = TS._set_walls(step, shape, walls)
        return ref, np.asarray(ref[1], bool)
    kinds = {}
    for end, sign in ((0, 1), (-1, -1)):
        n = TN._unit(D, 1, sign)
        bc = lbm.FreeSlip(n)
        step.set_boundary_including_adjoint(bc, TN._end(D, 1, end))
        kinds[step.boundary_handling.conditions[bc]] = ('freeslip', n)
    ids = step.boundary_handling.flags.astype(np.int64)
    assert step._lattice_kernels().programs is not None
    return ('links', ids, kinds), ids != 0


def _step(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, force=None, layout='fzyx',
          field=False, cs=None, zc=False, schedule='lattice', walls=None, sigma='field'):
    rule, s, w = _rule(stencil, compressible, dtype, method, fm, force, layout, field, cs, zc, sigma)
    with TO._schedule_env(schedule):
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target=target,
                                                relaxation_rate=None if field else OMEGA)
    assert (step._lattice is not None) == (schedule == 'lattice')
    if schedule == 'lattice' and sigma == 'field':
        assert step._solid_field == s and step._lattice_kernels().solid_field and step._lattice_kernels().spec.sf
    ref_walls, wall = (None, None) if walls is None else _set_walls(step, shape, walls)
    return step, ref_walls, wall


def _sigma(shape, seed, wall=None):
    """σ uniform in (0.05, 0.95), three fluid cells at exactly 0 and three at exactly 1."""
    rng = np.random.default_rng(seed + 7)
    S = rng.uniform(0.05, 0.95, shape)
    fluid = np.flatnonzero(~wall.ravel()) if wall is not None else np.arange(S.size)
    pick = rng.choice(fluid, 6, replace=False)
    S.ravel()[pick[:3]] = 0.0
    S.ravel()[pick[3:]] = 1.0
    return S


_REFS = {}


def _case(stencil, shape, compressible, target, dtype='float64', method='srt', fm=None, force_kind=None, layout='fzyx',
          walls=None, field=False, cs=None, zc=False, schedule='lattice', T=3, seed=11):
    """The timestep op against the reference (computed once per case and shared): (got, reference) pairs of the pdfs
    ``out``, the pdf adjoint ``gx``, the σ adjoint ``gS`` (and ``gW`` / ``gF``), as float64 CPU tensors."""
    import torch
    D = len(shape)
    F = ps.fields(f'F({D}): {dtype}[{D}D]') if force_kind == 'field' else None
    force = F if F is not None else FORCE[D] if fm is not None else None
    step, ref_walls, wall = _step(stencil, shape, compressible, target, dtype, method, fm, force, layout, field, cs, zc,
                                  schedule, walls)
    names = [f.name for f in step._additional_fields]
    assert names == [nm for nm, on in (('F', F is not None), ('omega_f', field), ('sigma', True)) if on]   # by name
    op = step.create_timestep_op(T)
    f0 = _init(stencil, shape, compressible, seed=seed + 1)
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.6, 1.9, shape)
    g = rng.standard_normal(f0.shape)
    Fv = 1e-3 * rng.standard_normal(shape + (D,))
    S = _sigma(shape, seed, wall)
    wts = np.array([float(v) for v in OL.SETS[stencil][1]])
    dev = 'cuda' if target == 'gpu' else 'cpu'
    tdt = getattr(torch, dtype)
    # (the reference runs on the inputs as the kernels see them: rounded to the pdf dtype)
    x = torch.tensor(f0 - wts if zc else f0, dtype=tdt, device=dev, requires_grad=True)
    St = torch.tensor(S, dtype=tdt, device=dev, requires_grad=True)
    Wt = torch.tensor(W, dtype=tdt, device=dev, requires_grad=True) if field else None
    Ft = torch.tensor(Fv, dtype=tdt, device=dev, requires_grad=True) if F is not None else None
    gt = torch.tensor(g, dtype=tdt, device=dev)
    assert bool((St == 0).any()) and bool((St == 1).any())
    extras = [t for t in (Ft, Wt, St) if t is not None]
    out = op.apply(x, *extras)
    out.backward(gt)
    key = (stencil, shape, compressible, dtype, method, fm, force_kind, walls, field, cs, zc, T, seed)
    if key not in _REFS:
        xr, Sr = x.detach().double().cpu().requires_grad_(), St.detach().double().cpu().requires_grad_()
        Wr = Wt.detach().double().cpu().requires_grad_() if field else None
        Fr = Ft.detach().double().cpu().requires_grad_() if F is not None else None
        rw = None if ref_walls is None else (ref_walls[0],) + tuple(
            torch.tensor(a) if isinstance(a, np.ndarray) else a for a in ref_walls[1:])
        rforce = tuple(Fr[..., a] for a in range(D)) if F is not None else force
        Wref = Wr if field else torch.full(shape, OMEGA, dtype=torch.float64)
        ref = _reference_states(xr + torch.tensor(wts) if zc else xr, Sr, Wref, T, stencil, compressible, method, fm,
                                rforce, rw, cs)[-1]
        ins = [t for t in (xr, Fr, Wr, Sr) if t is not None]
        grads = torch.autograd.grad(ref, ins, gt.double().cpu())
        _REFS[key] = (ref.detach() - (torch.tensor(wts) if zc else 0), [t.detach() for t in grads])
    ref, grads = _REFS[key]
    res = dict(out=(out.detach().double().cpu(), ref), gx=(x.grad.double().cpu(), grads[0]))
    for nm, t, gr in zip([n for n, on in (('gF', F is not None), ('gW', field), ('gS', True)) if on], extras, grads[1:]):
        res[nm] = (t.grad.double().cpu(), gr)
    assert float(res['gS'][1].abs().max()) > 0
    res.update(step=step, wall=wall, ref_walls=ref_walls, inputs=(x, extras, gt))
    return res


def _check(res, tol, gtol, names=('out', 'gx', 'gS', 'gW', 'gF')):
    for name in names:
        if name in res:
            got, ref = res[name]
            t = gtol if name.startswith('g') else tol
            err, scale = float((got - ref).abs().max()), float(ref.abs().max())
            print(f'{name}: max error {err:.3e} of max {scale:.3e} (ratio {err / scale:.3e}, bound {t:.0e})')
            assert scale > 0 and err <= t * scale, (name, err, scale)
    wall = res.get('wall')
    if wall is not None and 'gS' in res:
        # obstacle cells: dσ is exactly 0, in the kernels and in the reference
        assert wall.any() and float(res['gS'][0][wall].abs().max()) == 0.0
        assert float(res['gS'][1][wall].abs().max()) == 0.0


# --- the rule --------------------------------------------------------------------------------------------------
def test_rule_keyword():
    """``solid_fraction=None`` / ``False``: the rule as it stands, assignment for assignment. A number in [0, 1], a symbol
    or a field expression: the subexpression ``solid_fraction`` carries σ, ``ac.solid_fraction`` keeps the expression and
    every main assignment reads it; a field with an index dimension or a number outside [0, 1] is a ``ValueError``."""
    for kw in (dict(), dict(method='trt'), dict(method='mrt', relaxation_rates=[sp.Symbol('omega'), 1.1]),
               dict(force_model='guo', force=(1e-3, 2e-3)), dict(smagorinsky=0.2), dict(zero_centered=True)):
        plain = lbm.create_lb_update_rule('D2Q9', compressible=True, **kw)
        for off in (False, None):
            rule = lbm.create_lb_update_rule('D2Q9', compressible=True, solid_fraction=off, **kw)
            assert [str(a) for a in rule.all_assignments] == [str(a) for a in plain.all_assignments]
            assert rule.solid_fraction is None
    assert plain.solid_fraction is None
    s = ps.fields('s: float64[2D]')
    sym = sp.Symbol('sigma_0')
    for value, want in ((0.25, sp.sympify(0.25)), (0, sp.Integer(0)), (1, sp.Integer(1)), (sym, sym),
                        (s.center, s.center), (s, s.center), (s[1, 0] ** 2, s[1, 0] ** 2)):
        rule = lbm.create_lb_update_rule('D2Q9', solid_fraction=value)
        assert rule.solid_fraction == want
        sub = [a for a in rule.subexpressions if str(a.lhs) == 'solid_fraction']
        assert len(sub) == 1 and sub[0].rhs == want
        for a in rule.main_assignments:
            assert sp.Symbol('solid_fraction') in a.rhs.free_symbols
    for bad in (-0.1, 1.5, True):
        with pytest.raises(ValueError, match='solid_fraction'):
            lbm.create_lb_update_rule('D2Q9', solid_fraction=bad)
    sv = ps.fields('sv(2): float64[2D]')
    for bad in (sv.center(0), sv):
        with pytest.raises(ValueError, match='sv'):
            lbm.create_lb_update_rule('D2Q9', solid_fraction=bad)


def test_rule_is_the_blend_of_the_plain_rule():
    """Symbolically: ``dst_i − [(1 − σ) c_i + σ f_ī]`` is 0 with ``c_i`` the plain rule's right-hand side (D2Q9 SRT with
    a Guo force, zero-centred: the stored value is the blend minus ``w_i``)."""
    st = lbm.LBStencil('D2Q9')
    sg = sp.Symbol('sigma_0')
    kw = dict(compressible=True, force_model='guo', force=(sp.Rational(1, 700), sp.Rational(-1, 300)), zero_centered=True)
    src, dst = ps.fields('src(9), dst(9): float64[2D]', layout='fzyx')
    plain = lbm.create_lb_update_rule('D2Q9', src_field=src, dst_field=dst, **kw).new_without_subexpressions()
    rule = lbm.create_lb_update_rule('D2Q9', src_field=src, dst_field=dst, solid_fraction=sg,
                                     **kw).new_without_subexpressions()
    for i, (a, b) in enumerate(zip(rule.main_assignments, plain.main_assignments)):
        j = st.inverse_direction_index(i)
        w = st.weights[i]
        fj = src[tuple(-c for c in st.directions[j])](j) + st.weights[j]
        assert sp.simplify(a.rhs - ((1 - sg) * (b.rhs + w) + sg * fj - w)) == 0


# --- CPU: the lattice schedule ---------------------------------------------------------------------------------
#             stencil, shape, compressible, method, force model, force kind, layout, walls, ω field, C_s, zero-centred
CPU_LATTICE = [('D2Q9', (9, 7), True, 'srt', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), False, 'srt', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (12, 9), True, 'srt', None, None, 'fzyx', 'channel', False, None, False),
               ('D2Q9', (12, 9), False, 'trt-magic', None, None, 'fzyx', 'channel', True, None, False),
               ('D3Q19', (5, 4, 6), True, 'srt', None, None, 'fzyx', None, False, None, False),
               ('D3Q19', (5, 4, 6), False, 'mrt', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'trt-magic', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), False, 'trt-rate', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'mrt', None, None, 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'srt', 'guo', 'const', 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), False, 'srt', 'simple', 'const', 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'trt-magic', 'guo', 'const', 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'srt', 'guo', 'field', 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), False, 'srt', 'simple', 'field', 'fzyx', None, False, None, False),
               ('D2Q9', (9, 7), True, 'trt-magic', 'guo', 'field', 'fzyx', None, True, None, False),
               ('D2Q9', (9, 7), True, 'srt', None, None, 'fzyx', None, True, None, False),
               ('D2Q9', (9, 7), True, 'mrt', None, None, 'fzyx', None, True, None, False),
               ('D2Q9', (9, 7), True, 'srt', None, None, 'fzyx', None, False, CS, False),
               ('D2Q9', (9, 7), True, 'trt-magic', 'guo', 'const', 'fzyx', None, True, CS, False),
               ('D2Q9', (9, 7), False, 'mrt', None, None, 'fzyx', None, False, CS, False),
               ('D2Q9', (9, 7), True, 'srt', None, None, 'fzyx', None, False, None, True),
               ('D2Q9', (12, 9), True, 'srt', 'guo', 'const', 'fzyx', 'channel', False, None, True),
               ('D2Q9', (9, 7), True, 'srt', None, None, 'numpy', None, False, None, False),
               ('D2Q9', (12, 9), True, 'srt', None, None, 'fzyx', 'pressure', False, None, False),
               ('D2Q9', (12, 9), False, 'srt', None, None, 'fzyx', 'pressure', True, None, False),
               ('D2Q9', (12, 9), True, 'srt', None, None, 'fzyx', 'slip', False, None, False),
               ('D3Q19', (5, 4, 6), True, 'srt', None, None, 'fzyx', 'slip', False, None, False)]


@pytest.mark.parametrize('stencil,shape,compressible,method,fm,force_kind,layout,walls,field,cs,zc', CPU_LATTICE)
def test_solid_fraction_lattice_cpu_vs_reference(stencil, shape, compressible, method, fm, force_kind, layout, walls,
                                                 field, cs, zc):
    """The C lattice kernels, float64, T = 3 through the timestep op: pdfs, pdf adjoint, ``dσ`` (and ``dω`` / ``dF``, in
    the order of the extras) against the reference at the ω-field tests' bounds (1e-13 outputs, 1e-12 gradients, of each
    array's maximum); obstacle cells get exactly 0."""
    res = _case(stencil, shape, compressible, 'cpu', method=method, fm=fm, force_kind=force_kind, layout=layout,
                walls=walls, field=field, cs=cs, zc=zc)
    _check(res, 1e-13, 1e-12)
    assert ('gW' in res) == field and ('gF' in res) == (force_kind == 'field')
    if walls:
        assert float(res['gS'][0][~res['wall']].abs().min()) > 0.0


# --- CPU: the AutoDiffOp schedule ------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['srt', 'trt-magic'])
def test_solid_fraction_autodiffop_cpu_vs_reference(method):
    """``PSAD_LBM_LATTICE=0``: the σ field on the rule's AutoDiffOp kernels (the generic transposed derivation, an
    implementation independent of the lattice kernels' ``solid_adjoint``)."""
    res = _case('D2Q9', (8, 6), True, 'cpu', method=method, schedule='autodiffop')
    _check(res, 1e-13, 1e-12)


# --- dσ and the blended v_j against the symbolic rule ----------------------------------------------------------
@pytest.mark.parametrize('smag', [False, True])
@pytest.mark.parametrize('guo', [False, True])
@pytest.mark.parametrize('method', ['srt', 'trt-magic', 'mrt'])
def test_dsigma_and_blended_scatter_match_the_symbolic_rule(method, guo, smag):
    """One adjoint step of the emitted C kernels on a 3×3 periodic lattice against ``Σ_i g_i ∂dst_i/∂f_k`` (the blended
    ``v_k``) and ``Σ_i g_i ∂dst_i/∂σ`` (``dσ``) with sympy's derivatives of the rule's assignments — the chain rule
    through the subexpressions, in their order — at the same random float64 numbers: 1e-11 of each maximum."""
    st = lbm.LBStencil('D2Q9')
    shape = (3, 3)
    Fc = FORCE[2] if guo else None
    rule, s, _ = _rule('D2Q9', True, method=method, fm='guo' if guo else None, force=Fc, cs=CS if smag else None)
    lhs = {a.lhs for a in rule.all_assignments}
    acc = sorted({x for a in rule.all_assignments for x in a.rhs.atoms(ps.Field.Access)} - lhs - {s.center}, key=str)
    f = [next(a for a in acc if tuple(a.index) == (i,)) for i in range(9)]            # the pulled pdfs src_i(x − c_i)
    assert len(acc) == 9 and all(tuple(int(o) for o in f[i].offsets) == tuple(-c for c in st.directions[i])
                                 for i in range(9))
    om = sp.Symbol('omega')
    var = f + [s.center]
    order = list(rule.subexpressions) + list(rule.main_assignments)
    parts = []
    for a in order:
        reads = sorted((x for x in a.rhs.free_symbols | a.rhs.atoms(ps.Field.Access) if x in lhs or x in var), key=str)
        parts.append((a.lhs, reads, sp.lambdify(reads + [om], [a.rhs] + [sp.diff(a.rhs, x) for x in reads], 'math')))

    def jacobian(*args):
        vals = dict(zip(var, args[:10]))
        grad = {x: np.eye(10)[k] for k, x in enumerate(var)}
        rows = []
        for name, reads, fn in parts:
            r = fn(*[vals[x] for x in reads], args[10])
            vals[name], grad[name] = r[0], sum((d * grad[x] for d, x in zip(r[1:], reads)), np.zeros(10))
            if isinstance(name, ps.Field.Access):
                rows.append(grad[name])
        return np.array(rows)
    f0, _, g = TS._inputs('D2Q9', shape, True, 5)
    S = np.random.default_rng(6).uniform(0.05, 0.95, shape)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA)
    assert step._lattice is not None
    step.set_pdfs(f0)
    step.run(1, record=True, extra={'sigma': S})
    dS = np.zeros_like(S)
    step.set_adjoint_pdfs(g)
    step.run_backward(1, extra={'sigma': S}, extra_adj={'diffsigma': dS})
    got = np.array(step.adjoint_pdf_array)
    want, wantS = np.zeros_like(f0), np.zeros_like(S)
    for y in range(3):
        for x in range(3):
            cell = [((y - c[0]) % 3, (x - c[1]) % 3) for c in st.directions]      # where f_k was pulled from
            J = np.array(jacobian(*[f0[cell[k] + (k,)] for k in range(9)], S[y, x], OMEGA), dtype=np.float64)
            v = g[y, x] @ J
            for k in range(9):
                want[cell[k] + (k,)] = v[k]
            wantS[y, x] = v[9]
    for name, a, b in (('v', got, want), ('dsigma', dS, wantS)):
        err, scale = np.abs(a - b).max(), np.abs(b).max()
        print(f'{method} guo={guo} smagorinsky={smag}: {name} max error {err:.3e} of {scale:.3e}')
        assert scale > 0 and err <= 1e-11 * scale


# --- known answers (periodic, plain pdfs) ----------------------------------------------------------------------
def _run_op(step, T, f0, S, g=None):
    import torch
    x, St = torch.tensor(f0, requires_grad=True), torch.tensor(S, requires_grad=True)
    out = step.create_timestep_op(T).apply(x, St)
    if g is not None:
        out.backward(torch.tensor(g))
    return out.detach().numpy(), (None if g is None else x.grad.numpy()), (None if g is None else St.grad.numpy())


@pytest.mark.parametrize('stencil,shape,method', [('D2Q9', (9, 7), 'srt'), ('D3Q19', (5, 4, 6), 'mrt')])
def test_full_solid_returns_the_input_after_two_steps(stencil, shape, method):
    """σ ≡ 1: every arriving population is returned reversed, so two steps give back the input, bit for bit."""
    step, _, _ = _step(stencil, shape, True, 'cpu', method=method)
    f0 = _init(stencil, shape, True, seed=3)
    out, _, _ = _run_op(step, 2, f0, np.ones(shape))
    assert np.array_equal(out, f0)
    once, _, _ = _run_op(step, 1, f0, np.ones(shape))
    assert np.array_equal(once, OL.stream(f0, stencil, np)[..., OL.inverse(stencil)]) and not np.array_equal(once, f0)


@pytest.mark.parametrize('method,fm', [('srt', None), ('trt-magic', 'guo'), ('mrt', None)])
def test_mass_is_conserved_for_any_sigma(method, fm):
    """Σ over cells and directions is conserved to 1e-13 relative, whatever σ is."""
    shape = (9, 7)
    step, _, _ = _step('D2Q9', shape, True, 'cpu', method=method, fm=fm, force=FORCE[2] if fm else None)
    f0 = _init('D2Q9', shape, True, seed=4)
    out, _, _ = _run_op(step, 5, f0, _sigma(shape, 4))
    assert abs(out.sum() - f0.sum()) <= 1e-13 * abs(f0.sum())


@pytest.mark.parametrize('method', ['srt', 'trt-magic'])
def test_zero_sigma_field_is_the_rule_without_the_keyword(method):
    """A σ ≡ 0 field: outputs and ``gx`` equal those of the rule without the keyword, to the float64 bounds."""
    import torch
    shape, T = (9, 7), 3
    f0 = _init('D2Q9', shape, True, seed=5)
    g = np.random.default_rng(5).standard_normal(f0.shape)
    step, _, _ = _step('D2Q9', shape, True, 'cpu', method=method)
    out, gx, gS = _run_op(step, T, f0, np.zeros(shape), g)
    plain, _, _ = _step('D2Q9', shape, True, 'cpu', method=method, sigma=None)
    assert plain._additional_fields == [] and plain._solid_field is None
    x = torch.tensor(f0, requires_grad=True)
    ref = plain.create_timestep_op(T).apply(x)
    ref.backward(torch.tensor(g))
    assert np.abs(out - ref.detach().numpy()).max() <= 1e-13 * np.abs(out).max()
    assert np.abs(gx - x.grad.numpy()).max() <= 1e-12 * np.abs(gx).max()
    assert np.abs(gS).max() > 0


# --- macroscopic outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('compressible,fm,walls', [(True, None, None), (False, 'guo', None), (True, None, 'channel')])
def test_macroscopic_outputs_with_a_sigma_field(compressible, fm, walls):
    """``create_timestep_op(4, macroscopic_outputs=2)``: ρ and u are those of the stored (blended) state, and their seeds
    reach ``gx`` and ``dσ``."""
    import torch
    stencil, shape, T, k = 'D2Q9', (12, 9) if walls else (9, 7), 4, 2
    D, n = 2, T // k
    force = FORCE[2] if fm else None
    step, ref_walls, wall = _step(stencil, shape, compressible, 'cpu', fm=fm, force=force, walls=walls)
    op = step.create_timestep_op(T, macroscopic_outputs=k)
    f0 = _init(stencil, shape, compressible, seed=8)
    S = _sigma(shape, 8, wall)
    rng = np.random.default_rng(9)
    c, a, b = rng.standard_normal(f0.shape), rng.standard_normal((n,) + shape), rng.standard_normal((n,) + shape + (D,))
    x, St = torch.tensor(f0, requires_grad=True), torch.tensor(S, requires_grad=True)
    out, rho, vel = op.apply(x, St)
    torch.autograd.backward([out, rho, vel], [torch.tensor(c), torch.tensor(a), torch.tensor(b)])
    xr, Sr = torch.tensor(f0, requires_grad=True), torch.tensor(S, requires_grad=True)
    rw = None if ref_walls is None else (ref_walls[0],) + tuple(torch.tensor(v) for v in ref_walls[1:])
    states = _reference_states(xr, Sr, torch.full(shape, OMEGA, dtype=torch.float64), T, stencil, compressible,
                               fm=fm, force=force, walls=rw)
    fluid = torch.ones(shape, dtype=torch.bool) if wall is None else torch.tensor(~wall)
    mom = [TM._moments(states[j * k - 1], stencil, compressible, fm, force) for j in range(1, n + 1)]
    rho_r = torch.stack([torch.where(fluid, r, torch.zeros_like(r)) for r, _ in mom])
    vel_r = torch.stack([torch.where(fluid[..., None], u, torch.zeros_like(u)) for _, u in mom])
    loss = (torch.tensor(c) * states[-1]).sum() + (torch.tensor(a) * rho_r).sum() + (torch.tensor(b) * vel_r).sum()
    gx, gS = torch.autograd.grad(loss, (xr, Sr))
    assert float(gS.abs().max()) > 0
    _check(dict(out=(out.detach(), states[-1].detach()), rho=(rho.detach(), rho_r.detach()),
                vel=(vel.detach(), vel_r.detach()), gx=(x.grad, gx), gS=(St.grad, gS), wall=wall), 1e-13, 1e-12,
           names=('out', 'rho', 'vel', 'gx', 'gS'))


# --- the public interface --------------------------------------------------------------------------------------
def test_sigma_field_run_and_run_backward():
    """``run`` / ``run_backward(extra=…, extra_adj=…)`` take the field and its adjoint array like the ω field's."""
    import torch
    shape, T = (9, 7), 3
    step, _, _ = _step('D2Q9', shape, True, 'cpu')
    f0, S = _init('D2Q9', shape, True, seed=41), _sigma(shape, 41)
    g = np.random.default_rng(41).standard_normal(f0.shape)
    step.set_pdfs(f0)
    step.run(T, record=True, extra={'sigma': S})
    dS = np.zeros_like(S)
    step.set_adjoint_pdfs(g)
    step.run_backward(T, extra={'sigma': S}, extra_adj={'diffsigma': dS})
    xr, Sr = torch.tensor(f0, requires_grad=True), torch.tensor(S, requires_grad=True)
    ref = _reference_states(xr, Sr, torch.full(shape, OMEGA, dtype=torch.float64), T, 'D2Q9', True)[-1]
    gx, gS = torch.autograd.grad(ref, (xr, Sr), torch.tensor(g))
    _check(dict(out=(torch.tensor(step.pdf_array), ref.detach()), gx=(torch.tensor(step.adjoint_pdf_array), gx),
                gS=(torch.tensor(dS), gS)), 1e-13, 1e-12)


def test_sigma_field_end_to_end_op():
    """``create_end_to_end_op(additional_fields_to_tensor_map={s: S})``: the tensor reaches every step; dloss/dσ at three
    cells against central differences (the bound of ``test_omega_field_end_to_end_op``)."""
    import torch
    shape = (9, 7)
    rule, s, _ = _rule('D2Q9', True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA)
    assert step._lattice is not None
    rng = np.random.default_rng(1)
    rho = torch.tensor(1 + 0.01 * rng.standard_normal(shape))
    vel = torch.tensor(0.03 * rng.standard_normal(shape + (2,)))
    St = torch.tensor(_sigma(shape, 1), requires_grad=True)

    def loss(Sv):
        r = step.create_end_to_end_op(4, vel, rho, additional_fields_to_tensor_map={s: Sv},
                                      num_times_steps_without_save=1)
        return (r.output_velocity_tensor ** 2).sum() + ((r.output_density_tensor - 1) ** 2).sum()
    loss(St).backward()
    e = 1e-6
    for idx in ((3, 2), (0, 6), (8, 0)):
        Sp, Sm = St.detach().clone(), St.detach().clone()
        Sp[idx] += e
        Sm[idx] -= e
        fd = (float(loss(Sp)) - float(loss(Sm))) / (2 * e)
        assert abs(fd - float(St.grad[idx])) <= 1e-6 * abs(fd) + 1e-9, (idx, fd, float(St.grad[idx]))
    with pytest.raises(ValueError, match='sigma'):
        step.create_end_to_end_op(4, vel, rho)


def test_scalar_sigma_through_expand():
    """A trainable scalar σ: ``s0.expand(*domain)`` as the field tensor; its gradient is the sum of ``gS``."""
    import torch
    shape, T = (9, 7), 3
    step, _, _ = _step('D2Q9', shape, True, 'cpu')
    op = step.create_timestep_op(T)
    f0 = _init('D2Q9', shape, True, seed=31)
    g = torch.tensor(np.random.default_rng(31).standard_normal(f0.shape))
    s0 = torch.tensor(0.37, dtype=torch.float64, requires_grad=True)
    op.apply(torch.tensor(f0), s0.expand(*shape)).backward(g)
    Sf = torch.full(shape, 0.37, dtype=torch.float64, requires_grad=True)
    op.apply(torch.tensor(f0), Sf).backward(g)
    total = float(Sf.grad.sum())
    assert s0.grad.shape == () and total != 0 and abs(float(s0.grad) - total) <= 1e-12 * abs(total)


# --- routing and errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['number', 'symbol', 'offset', 'dtype'])
def test_other_sigma_expressions_take_the_autodiffop_schedule(what):
    """A number, a symbol, a σ read at an offset or from a field of another dtype is not the lattice kernels' case:
    ``step._lattice is None``, and the rule's AutoDiffOp kernels compute the blend (one step against the reference)."""
    import torch
    shape = (6, 5)
    s = ps.fields('s: float32[2D]') if what == 'dtype' else ps.fields('s: float64[2D]')
    sigma = {'number': 0.25, 'symbol': sp.Symbol('sigma_0'), 'offset': s[1, 0], 'dtype': s.center}[what]
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, solid_fraction=sigma)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA,
                                            kernel_params={'sigma_0': 0.25} if what == 'symbol' else None)
    assert step._lattice is None and step._solid_field is None
    assert step._additional_fields == ([s] if what in ('offset', 'dtype') else [])
    # (not the structured adjoint rule, which knows no blend)
    assert step._autodiff_args['backward_assignments'] is None
    if what in ('number', 'symbol'):
        f0 = _init('D2Q9', shape, True, seed=2)
        step.set_pdfs(f0)
        step.run(1)
        ref = _reference_states(torch.tensor(f0), torch.full(shape, 0.25, dtype=torch.float64),
                                torch.full(shape, OMEGA, dtype=torch.float64), 1, 'D2Q9', True)[-1].numpy()
        assert np.abs(np.asarray(step.pdf_array) - ref).max() <= 1e-13 * np.abs(ref).max()


def test_float16_pdfs_with_a_sigma_field_run_on_the_generic_kernels():
    shape = (6, 5)
    st = lbm.LBStencil('D2Q9')
    rule, s, _ = _rule('D2Q9', True, dtype='float16', zc=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu', relaxation_rate=OMEGA)
    assert step._lattice is None and step._additional_fields == [s]
    wts = np.array([float(v) for v in st.weights])
    f0 = _init('D2Q9', shape, True, seed=2)
    step.set_pdfs((f0 - wts).astype(np.float16))
    step.run(1, extra={'sigma': _sigma(shape, 2).astype(np.float16)})
    assert np.isfinite(np.asarray(step.pdf_array, dtype=np.float64)).all()
    with pytest.raises(NotImplementedError, match='float16 pdfs: a per-cell solid-fraction field is not built'):
        LatticeSource(st, True, 'float', False, half=True, solid_field=True)
    with pytest.raises(NotImplementedError, match='float16'):
        LK.LatticeKernels(st, True, np.float16, False, 'cpu', solid_field=True)


def test_sigma_field_errors():
    """Wrong shape, wrong dtype, missing tensor, missing adjoint array, wrong strides; kernels without the field refuse
    one."""
    import torch
    shape = (9, 7)
    step, _, _ = _step('D2Q9', shape, True, 'cpu')
    op = step.create_timestep_op(2)
    f0, S = _init('D2Q9', shape, True, seed=51), _sigma(shape, 51)
    x = torch.tensor(f0)
    with pytest.raises(ValueError, match='solid-fraction field of shape'):
        op.apply(x, torch.tensor(S[:-1]))
    with pytest.raises(ValueError, match='solid-fraction field dtype'):
        op.apply(x, torch.tensor(S, dtype=torch.float32))
    with pytest.raises(TypeError, match='sigma'):
        op.apply(x)
    step.set_pdfs(f0)
    # (the same kind of message as a missing ω tensor)
    with pytest.raises(ValueError, match="reads the solid-fraction field 'sigma': pass its array"):
        step.run(1)
    wstep, _ = TO._step('D2Q9', shape, True, 'cpu')
    wstep.set_pdfs(f0)
    with pytest.raises(ValueError, match="reads the relaxation-rate field 'omega_f': pass its array"):
        wstep.run(1)
    step.run(1, record=True, extra={'sigma': S})
    with pytest.raises(ValueError, match='diffsigma'):
        step.run_backward(1, extra={'sigma': S})
    with pytest.raises(ValueError, match='strides'):
        step.run_backward(1, extra={'sigma': S}, extra_adj={'diffsigma': np.zeros(shape[::-1]).T})
    K = LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float64, False, 'cpu')
    src, dst = np.ascontiguousarray(f0), np.empty_like(f0)
    with pytest.raises(ValueError, match='no solid-fraction field'):
        K.forward(src, dst, 1.0, sof=S)
    Ks = LK.LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float64, False, 'cpu', solid_field=True)
    with pytest.raises(ValueError, match='need the solid-fraction field'):
        Ks.forward(src, dst, 1.0)


# --- the sources -----------------------------------------------------------------------------------------------
def test_argument_table_carries_the_group():
    """``LatticeSource(solid_field=True)`` adds one operand group: the σ pointer (and ``dsolid`` for the adjoint) after
    the ω field's, three strides after the ω field's; off, the table is what it was."""
    st = lbm.LBStencil('D2Q9')
    base = dict(stencil=st, compressible=True, ctype='double', walls=True, omega_field=True)
    on, off = LatticeSource(solid_field=True, **base), LatticeSource(**base)
    for kernel in ('fwd', 'adj'):
        t_on, t_off = kernel_args(on, kernel), kernel_args(off, kernel)
        group = [a for a in t_on if a.group == 'solid']
        assert [a.name for a in group] == (['sigf', 'dsolid'] if kernel == 'adj' else ['sigf']) + ['p_z', 'p_y', 'p_x']
        assert [a for a in t_on if a.group != 'solid'] == list(t_off)
        names = [a.name for a in t_on]
        assert names.index('sigf') == names.index('omf') + (2 if kernel == 'adj' else 1)
        assert names.index('p_z') == names.index('w_x') + 1
        assert group[0].decl == 'const T* __restrict__ sigf'
    assert kernel_args(on, 'adj')[[a.name for a in kernel_args(on, 'adj')].index('dsolid')].decl == \
        'T* __restrict__ dsolid'


def test_flag_off_changes_no_source():
    """``solid_field=False`` is the default: the emitted text is the same object's text, and the flag's lines are only
    in the variant's source."""
    from pystencils_autodiff_amd.lbm._lattice_source import emit
    st = lbm.LBStencil('D2Q9')
    for kw in (dict(), dict(omega_field=True), dict(mrt=None, trt=('magic', 3 / 16)), dict(smagorinsky=0.2)):
        base = dict(stencil=st, compressible=True, ctype='double', walls=True, **kw)
        off, on = emit(LatticeSource(**base)), emit(LatticeSource(solid_field=True, **base))
        assert off == emit(LatticeSource(solid_field=False, **base))
        for word in ('sfr', 'sigf', 'dsolid', 'dsf', 'p_x'):
            assert word not in off and word in on
        assert on.count('dsolid[pc] += (T)dsf;') == 1


_SOURCE_KERNELS = {}


def _source_kernels(variant):
    """The HIP ``LatticeKernels`` of a σ-field family with link programs (a FixedDensity channel), made once."""
    if variant not in _SOURCE_KERNELS:
        K = _step('D2Q9', (9, 8), True, 'gpu', 'float32', field=variant == 'omega',
                  cs=CS if variant == 'smagorinsky' else None, walls='pressure')[0]._lattice_kernels()
        assert K.solid_field and K.programs is not None
        _SOURCE_KERNELS[variant] = K
    return _SOURCE_KERNELS[variant]


@pytest.mark.parametrize('fix', [False, True])
@pytest.mark.parametrize('addr', ['buf', 'ptr'])
@pytest.mark.parametrize('idx', ['int', 'long long'])
@pytest.mark.parametrize('variant', ['plain', 'omega', 'smagorinsky', 'macroscopic'])
def test_solid_fraction_sources_compile(monkeypatch, variant, idx, addr, fix):
    """(``int`` / ``long long``) × (``buf`` / ``ptr``) × (main / fix-up), plain, with the ω field, with Smagorinsky and
    the density / velocity variant, compile to gfx950 code objects; every source loads σ once per cell function and adds
    ``dσ`` once."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from tests.test_native_abi import _is_amdgpu_elf
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    K = _source_kernels(variant)
    src = K.source(idx, addr, fix=fix, macro=variant == 'macroscopic')
    assert src.count('const float sfr = (float)sigf[pc], sfr1 = (float)1 - sfr;') == 2
    assert src.count('dsolid[pc] += (T)dsf;') == 1
    assert src.count('domega[wc] +=') == int(variant == 'omega')
    assert ('rho_out[rc] = mo_r;' in src) == (variant == 'macroscopic')
    code = rt.compile_hip(src, name='psad_lbm.hip')
    assert _is_amdgpu_elf(code)
    for nm in (['lbm_adj_fix'] if fix else ['lbm_fwd', 'lbm_adj']):
        assert nm.encode() in code
    # pointers: 3 pdf arrays, mask, ids, (omf, domega,) sigf, dsolid(, 4 macroscopic arrays); strides: 3 × 4 (+ 3) + 3
    sig = src[src.index('lbm_adj_fix(' if fix else 'lbm_adj('):]
    sig = sig[:sig.index(')')]
    assert sig.count('*') == 7 + 2 * int(variant == 'omega') + 4 * int(variant == 'macroscopic') + int(fix)
    assert sig.count('const IDX') == 15 + 3 * int(variant == 'omega') + 7 * int(variant == 'macroscopic')


def test_solid_fraction_source_variants_differ_and_c_builds():
    K = _source_kernels('plain')
    assert len({K.source(idx, addr, fix=fix) for idx in ('int', 'long long') for addr in ('buf', 'ptr')
                for fix in (False, True)}) == 8
    Kc = _step('D2Q9', (9, 8), True, 'cpu', 'float32', field=True, walls='pressure')[0]._lattice_kernels()
    assert Kc.build() is not None and Kc.build(macro=True) is not None
    # a σ field that reaches 2³¹ − 1 elements widens the index type alone; the plan's key tells σ layouts apart
    import torch
    pdfs = [torch.empty((6, 5, 9), dtype=torch.float32, device='meta')] * 3
    far = torch.empty_strided((6, 5), (2 ** 31 // 5, 1), dtype=torch.float32, device='meta')
    near = torch.empty((6, 5), dtype=torch.float32, device='meta')
    assert K._launch_mode(pdfs, {'solid': (near, near)}) == ('int', 'buf')
    assert K._launch_mode(pdfs, {'solid': (far, far)}) == ('long long', 'buf')
    assert K._launch_mode(pdfs, {'solid': (near, far)}) == ('long long', 'buf')


# --- GPU -------------------------------------------------------------------------------------------------------
#          stencil, shape, compressible, method, force model, force kind, ω field
GPU_F64 = [('D2Q9', (64, 48), True, 'srt', None, None, False),             # 12 blocks: the XCD remap has a remainder
           ('D3Q19', (20, 17, 70), False, 'mrt', None, None, False),
           ('D2Q9', (64, 48), True, 'trt-magic', 'guo', 'field', True)]


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape,compressible,method,fm,force_kind,field', GPU_F64)
def test_solid_fraction_lattice_gpu_vs_reference(stencil, shape, compressible, method, fm, force_kind, field):
    """The HIP lattice kernels in float64 at the CPU bounds (1e-13 outputs, 1e-12 gradients)."""
    res = _case(stencil, shape, compressible, 'gpu', method=method, fm=fm, force_kind=force_kind, field=field)
    _check(res, 1e-13, 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('walls', ['pressure', 'slip'])
def test_solid_fraction_fixup_launch_gpu(walls):
    """Link-program walls, D2Q9 (70, 33): the listed cells' ``dσ`` comes from the fix-up launch — equal to the reference
    there; ``dσ`` at obstacle cells is 0; a second backward gives bitwise the same ``dσ``."""
    import torch
    shape = (70, 33)
    res = _case('D2Q9', shape, True, 'gpu', walls=walls)
    _check(res, 1e-13, 1e-12)
    step = res['step']
    cells = step._cells_arg()
    assert cells is not None and int(cells.numel()) > 0
    listed = np.zeros(int(np.prod(shape)), bool)
    listed[cells.cpu().numpy()] = True
    listed = torch.tensor(listed.reshape(shape))
    got, ref = res['gS']
    assert float(ref[listed].abs().min()) > 0
    assert float((got[listed] - ref[listed]).abs().max()) <= 1e-12 * float(ref.abs().max())
    wall = torch.tensor(res['wall'])
    assert bool(wall.any()) and float(got[wall].abs().max()) == 0.0
    x, (St,), gt = res['inputs']
    again = []
    for _ in range(2):
        x.grad = St.grad = None
        step.create_timestep_op(3).apply(x, St).backward(gt)
        again.append(St.grad.clone())
    assert torch.equal(again[0], again[1]) and torch.equal(again[0].double().cpu(), got)


@pytest.mark.gpu
def test_solid_fraction_schedules_agree_gpu():
    """The lattice kernels against the rule's AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``) on the same inputs."""
    a = _case('D2Q9', (37, 70), True, 'gpu', schedule='lattice')
    b = _case('D2Q9', (37, 70), True, 'gpu', schedule='autodiffop')
    _check(b, 1e-13, 1e-12)
    _check({k: (a[k][0], b[k][0]) for k in ('out', 'gx', 'gS')}, 1e-13, 1e-12)


@pytest.mark.gpu
def test_solid_fraction_ptr_addressing_bitwise_gpu(monkeypatch):
    """``PSAD_LBM_ADDR=ptr``: bitwise equal to ``buf`` in float64."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    a = _case('D2Q9', (37, 70), False, 'gpu', layout='numpy', walls='channel')
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    b = _case('D2Q9', (37, 70), False, 'gpu', layout='numpy', walls='channel')
    assert {k[2] for k in b['step']._lattice_kernels()._fns} == {'ptr'}
    assert {k[2] for k in a['step']._lattice_kernels()._fns} == {'buf'}
    for k in ('out', 'gx', 'gS'):
        assert torch.equal(a[k][0], b[k][0]), k


def _chain_length(Q):
    """k of the per-cell bound: the longest dependent fp32 chain from loaded values to ``dσ`` in the emitted adjoint cell
    (SRT, compressible — the incompressible one is shorter). ``dsf`` first takes the pdf part, Q sequential statements
    ``dsf += (ω g_k + g_k̄ − g_k) f_k`` — a chain of Q + 4 — and then the Q sequential ``dsf −= (ω g_k) feq_k``, whose
    last operand is ready after ρ = f0 + … (Q − 1 adds), 1/ρ and u_a = m_a/ρ (2), c·u (1: at most two nonzero axes on
    D2Q9 / D3Q19), poly = cu (3 + 4.5 cu) − 1.5 u² (4), feq = (w ρ)(1 + poly) (2) and (ω g) · feq (1): the longer of the
    two, (Q − 1) + 10, plus the Q subtractions — 2 Q + 9, as for ``dω``. (The store ``dsolid += dsf`` onto the zeroed
    array is exact at T = 1.)"""
    return 2 * Q + 9


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape,compressible', [('D2Q9', (64, 48), True), ('D3Q19', (20, 17, 70), False)])
def test_solid_fraction_float32_gpu(stencil, shape, compressible):
    """float32, no-slip channel with an obstacle.
    (a) T = 1, per fluid cell: ``|dσ − ref| ≤ k 2⁻²⁴ Σ_i |g_i| (|f_ī| + |c_i|)`` (float64 reference), k =
    ``_chain_length``;
    (b) T = 3: for each of ``out``, ``gx``, ``gS`` the error against the float64 reference is at most 4× the error of
    the same reference evaluated in float32 on the CPU on the same inputs.
    Measured on an MI355X: see DESIGN.md, "Solid fraction"."""
    import torch
    Q = len(OL.SETS[stencil][0])
    inv = OL.inverse(stencil)
    # (a)
    res = _case(stencil, shape, compressible, 'gpu', 'float32', walls='channel', T=1)
    x, (St,), gt = res['inputs']
    wall = torch.tensor(res['wall'])
    fs = OL.stream_walls(x.detach().double().cpu(), stencil, wall, torch)
    c = TO._collide(fs, torch.full(shape, OMEGA, dtype=torch.float64), stencil, compressible, 'srt', None, None, torch)
    bound = _chain_length(Q) * 2.0 ** -24 * (gt.double().cpu().abs() * (fs[..., inv].abs() + c.abs())).sum(-1)
    got, ref = res['gS']
    err = (got - ref).abs()
    fluid = ~wall
    print(f'(a) {stencil}: worst |dsigma - ref| / bound = {float((err[fluid] / bound[fluid]).max()):.3f} '
          f'(k = {_chain_length(Q)}); |dsigma| max {float(ref.abs().max()):.3e}')
    assert bool((err[fluid] <= bound[fluid]).all()) and float(got[wall].abs().max()) == 0.0
    # (b)
    res = _case(stencil, shape, compressible, 'gpu', 'float32', walls='channel', T=3)
    x, (St,), gt = res['inputs']
    x32, S32 = x.detach().cpu().requires_grad_(), St.detach().cpu().requires_grad_()
    ref32 = _reference_states(x32, S32, torch.full(shape, OMEGA, dtype=torch.float32), 3, stencil, compressible,
                              walls=('noslip', wall))[-1]
    gx32, gS32 = torch.autograd.grad(ref32, (x32, S32), gt.cpu())
    ratios = {}
    for name, cpu32 in (('out', ref32.detach()), ('gx', gx32), ('gS', gS32)):
        got, ref = res[name]
        e_gpu, e_cpu = float((got - ref).abs().max()), float((cpu32.double() - ref).abs().max())
        ratios[name] = e_gpu / e_cpu
        print(f'(b) {stencil} {name}: error {e_gpu:.3e}, float32 reference {e_cpu:.3e}, ratio {e_gpu / e_cpu:.3f} '
              f'(bound 4)')
    assert all(r <= 4 for r in ratios.values()), ratios
    assert float(res['gS'][0][wall].abs().max()) == 0.0
