"""Walls whose links read neighbouring fluid cells (``lbm.NeighbourBoundary``: ``FreeSlip``, ``ZeroGradientOutflow``,
user links): the printed links and their derived adjoints, T steps and their adjoint on the C and HIP lattice kernels
against an array-roll restatement written here (streaming with the link rule and its bounce-back fallback,
``oracle/lbm.py``'s collision; the adjoint by torch's reverse mode through it), the free-slip fixed point, and the
emitted source of every lattice the kernels took before, which must not change."""
import hashlib
import json
import os

import numpy as np
import pytest
import sympy as sp

from oracle import lbm as OL
from pystencils_autodiff_amd import AdjointField, lbm, ps

OMEGA = 1.3
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'lattice_source_sha.json')
GOLDEN_ALL = os.path.join(os.path.dirname(__file__), 'golden', 'lattice_source_sha_all.json')


def _init(stencil, shape, compressible, seed=0):
    rng = np.random.default_rng(seed)
    D = len(shape)
    Q = len(OL.SETS[stencil][0])
    rho = 1 + 0.05 * rng.standard_normal(shape)
    u = 0.04 * rng.standard_normal(shape + (D,))
    return OL.equilibrium(rho, u, stencil, compressible) + 0.01 * rng.standard_normal(shape + (Q,))


class Mixed(lbm.NeighbourBoundary):
    """A user link, nonlinear in a neighbour's and the cell's own pdfs: the free-slip link times
    ``1 + 0.1 pdf(0)``."""

    def __init__(self, normal_direction):
        super().__init__('Mixed' + str(tuple(normal_direction)))
        self.slip = lbm.FreeSlip(normal_direction)

    def __call__(self, pdf_field, direction, lb_method, **kw):
        (a,) = self.slip(pdf_field, direction, lb_method)
        if a.rhs == pdf_field(direction):
            return [a]
        return [ps.Assignment(a.lhs, a.rhs * (1 + 0.1 * pdf_field(0)))]


# --- the restatement -------------------------------------------------------------------------------------------
def _shift(xp, a, c):
    """``a`` read at ``x + c`` (periodic)."""
    return OL._roll_all(xp, a, tuple(-int(v) for v in c))


def stream_links(f, stencil, ids, kinds, compressible, xp):
    """Pull streaming with walls: ``ids`` the wall ids over the domain (0: fluid), ``kinds[id]`` one of ``('noslip',)``,
    ``('freeslip', n)``, ``('outflow', n)``, ``('mixed', n)``, ``('pressure', ρ_w)``. Where ``x − c_i`` is a wall cell,
    with ``d = ī`` the direction that left ``x`` towards it: the wall's link, evaluated on the pre-streaming state;
    a link that reads ``x + o`` where that cell is not fluid is the bounce-back ``f_d(x)``."""
    dirs, w = OL.SETS[stencil]
    inv = OL.inverse(stencil)
    D = len(dirs[0])
    fluid = ids == 0
    comps = []
    for i, c in enumerate(dirs):
        pulled = OL._roll_all(xp, f[..., i], c)
        if not any(c):
            comps.append(pulled)
            continue
        d = inv[i]
        cd = dirs[d]
        nb_id = OL._roll_all(xp, ids, c)
        bounced = f[..., d]
        res = xp.where(nb_id != 0, bounced, pulled)
        for wid, kind in kinds.items():
            link = None
            if kind[0] in ('freeslip', 'mixed'):
                n = kind[1]
                s = sum(a * b for a, b in zip(cd, n))
                t = tuple(a - s * b for a, b in zip(cd, n))
                if s < 0 and any(t):
                    m = dirs.index(tuple(a - 2 * b for a, b in zip(cd, t)))
                    val = _shift(xp, f[..., m], t)
                    if kind[0] == 'mixed':
                        val = val * (1 + 0.1 * f[..., 0])
                    link = xp.where(_shift(xp, fluid, t), val, bounced)
            elif kind[0] == 'outflow':
                n = kind[1]
                if sum(a * b for a, b in zip(cd, n)) < 0:
                    link = xp.where(_shift(xp, fluid, n), _shift(xp, f[..., i], n), bounced)
            elif kind[0] == 'pressure':
                rw = kind[1]
                mom = [sum(ck[a] * f[..., k] for k, ck in enumerate(dirs) if ck[a]) for a in range(D)]
                u = [ma / rw if compressible else ma for ma in mom]
                cu = sum(cd[a] * u[a] for a in range(D) if cd[a])
                usq = sum(ua * ua for ua in u)
                sym = rw * (1 + 4.5 * cu * cu - 1.5 * usq) if compressible else rw + 4.5 * cu * cu - 1.5 * usq
                link = 2 * float(w[d]) * sym - f[..., d]
            if link is not None:
                res = xp.where(nb_id == wid, link, res)
        comps.append(res)
    return xp.stack(comps, -1) if xp.__name__ != 'torch' else xp.stack(comps, dim=-1)


def run_links(f, omega, ids, kinds, steps, stencil, compressible, xp, omega_odd=None, mrt=None):
    """``steps`` stream-pull-collide steps with the walls of ``stream_links``; wall cells keep their state."""
    wall = ids != 0
    keep = wall[..., None] if xp.__name__ != 'torch' else wall.unsqueeze(-1)
    for _ in range(steps):
        new = OL.collide(stream_links(f, stencil, ids, kinds, compressible, xp), omega, stencil, compressible, xp,
                         omega_odd=omega_odd, mrt=mrt)
        f = xp.where(keep, f, new)
    return f


# --- lattices --------------------------------------------------------------------------------------------------
MRT_RATES = dict(shear=OMEGA, bulk=1.1, third=0.9, fourth=1.2)


def _unit(D, axis, sign):
    return tuple(sign if a == axis else 0 for a in range(D))


def _end(D, axis, end, inner_axes=()):
    return tuple(end if a == axis else (slice(1, -1) if a in inner_axes else slice(None)) for a in range(D))


def _lattice(name, stencil, shape, target, dtype='float64', method='srt', compressible=True):
    """A step with the walls of lattice ``name``; returns (step, kinds, omega_odd, mrt matrix)."""
    D = len(shape)
    kw = {}
    w_odd = mrt = None
    if method == 'trt':
        kw, w_odd = dict(method='trt'), OL.trt_odd_rate(OMEGA)
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[sp.Symbol('omega'), MRT_RATES['bulk'], MRT_RATES['third'],
                                                  MRT_RATES['fourth']])
        mrt = OL.mrt_matrix(stencil, MRT_RATES)
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, **kw)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=OMEGA, target=target)
    kinds = {}

    def put(bc, kind, sl):
        step.set_boundary_including_adjoint(bc, sl)
        kinds[step.boundary_handling.conditions[bc]] = kind

    def sides(cls, kind, axis=1):
        for end, sign in ((0, 1), (-1, -1)):
            n = _unit(D, axis, sign)
            put(cls(n), (kind, n), _end(D, axis, end))
    if name == 'slip':                       # free-slip on both ends of axis 1, periodic along the others
        sides(lbm.FreeSlip, 'freeslip')
    elif name == 'mixed':
        sides(Mixed, 'mixed')
    elif name == 'outflow2':                 # copying outlets on both ends of axis 1: reads along the normal
        sides(lbm.ZeroGradientOutflow, 'outflow')
    elif name == 'box':                      # free-slip on axis 1, no-slip on axis 0: the fallback at the corners
        sides(lbm.FreeSlip, 'freeslip')
        for end in (0, -1):
            put(lbm.NoSlip(), ('noslip',), _end(D, 0, end))
    elif name == 'open':                     # pressure inlet, copying outlet, free-slip sides
        sides(lbm.FreeSlip, 'freeslip')
        put(lbm.FixedDensity(1.02, name='inlet'), ('pressure', 1.02), _end(D, 0, 0, (1,)))
        n = _unit(D, 0, -1)
        put(lbm.ZeroGradientOutflow(n), ('outflow', n), _end(D, 0, -1, (1,)))
    else:
        raise ValueError(name)
    return step, kinds, w_odd, mrt


_REFS = {}


def _reference(name, stencil, shape, method, compressible, T, kinds, ids, w_odd, mrt):
    """(f0, g, forward, adjoint) of the restatement in float64, computed once per lattice."""
    import torch
    key = (name, stencil, shape, method, compressible, T)
    if key not in _REFS:
        f0 = _init(stencil, shape, compressible, seed=51)
        g = np.random.default_rng(52).standard_normal(f0.shape)
        ft = torch.tensor(f0, requires_grad=True)
        ref = run_links(ft, OMEGA, torch.tensor(ids.astype(np.int64)), kinds, T, stencil, compressible, torch,
                        omega_odd=w_odd, mrt=mrt)
        (gref,) = torch.autograd.grad(ref, ft, torch.tensor(g))
        plain = run_links(torch.tensor(f0), OMEGA, torch.tensor(ids.astype(np.int64)),
                          {k: ('noslip',) for k in kinds}, T, stencil, compressible, torch, omega_odd=w_odd, mrt=mrt)
        # the links are in: the same walls bouncing back everywhere give another flow
        assert float((ref.detach() - plain).abs().max()) > 1e-4
        for a in (f0, g):
            a.setflags(write=False)
        _REFS[key] = f0, g, ref.detach().numpy(), gref.numpy()
    return _REFS[key]


# --- API -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stencil', ['D2Q9', 'D3Q19', 'D3Q27'])
def test_neighbour_boundary_links_and_adjoints(stencil):
    """``FreeSlip`` / ``ZeroGradientOutflow`` print the links of their docstrings (``m`` always in the stencil), and
    ``AdjointBoundaryCondition`` of each the transposed copy ``diffpdf[o](k) ← diffpdf[c_d](ī_d)``."""
    st = lbm.LBStencil(stencil)
    D, Q = st.D, st.Q
    dirs = [tuple(int(v) for v in c) for c in st.directions]
    f = ps.fields(f'f({Q}): [{D}D]')
    g = AdjointField(f)
    for axis in range(D):
        for sign in (1, -1):
            n = _unit(D, axis, sign)
            slip, out = lbm.FreeSlip(n), lbm.ZeroGradientOutflow(n)
            assert isinstance(slip, lbm.NeighbourBoundary) and isinstance(out, lbm.NeighbourBoundary)
            for d in range(1, Q):
                c = dirs[d]
                inv = st.inverse_direction_index(d)
                s = sum(a * b for a, b in zip(c, n))
                t = tuple(a - s * b for a, b in zip(c, n))
                (a,) = slip(f, d, st)
                assert a.lhs == f[c](inv)
                if s >= 0 or not any(t):
                    assert a.rhs == f(d)
                    o, k = (0,) * D, d
                else:
                    cm = tuple(x - 2 * y for x, y in zip(c, t))
                    assert cm in dirs and t in dirs
                    assert a.rhs == f[t](dirs.index(cm))
                    o, k = t, dirs.index(cm)
                (b,) = lbm.AdjointBoundaryCondition(slip)(g, d, st).all_assignments
                assert b.lhs == g[o](k) and sp.simplify(b.rhs - g[c](inv)) == 0
                (a,) = out(f, d, st)
                assert a.lhs == f[c](inv)
                o, k = ((0,) * D, d) if s >= 0 else (n, inv)
                assert a.rhs == f[o](k)
                (b,) = lbm.AdjointBoundaryCondition(out)(g, d, st).all_assignments
                assert b.lhs == g[o](k) and sp.simplify(b.rhs - g[c](inv)) == 0
    with pytest.raises(ValueError):
        lbm.FreeSlip((1,) * D)
    with pytest.raises(ValueError):
        lbm.ZeroGradientOutflow((0,) * D)


def test_neighbour_link_forms():
    """``link_form`` gives the third kind for a ``NeighbourBoundary`` (a user link, nonlinear in a neighbour's and the
    cell's pdfs, too) and leaves own-cell programs' tuples as they were; an offset outside the stencil raises, and a
    plain ``Boundary`` that reads another cell still does."""
    st = lbm.LBStencil('D2Q9')
    view = lbm.boundaries.LBMethodView(st, True)
    dirs = [tuple(c) for c in st.directions]
    slip = lbm.FreeSlip((0, 1))
    kind, prog = lbm.link_form(slip, lbm.AdjointBoundaryCondition(slip), view)
    assert kind == 'neighbour' and prog[0] is None
    for d in range(1, 9):
        s = dirs[d][1]
        if s >= 0 or dirs[d][0] == 0:
            assert prog[d] is None                     # the bounce-back: the fused table row
            continue
        lines, val, jac, offs = prog[d]
        t = dirs.index((dirs[d][0], 0))
        m = dirs.index((-dirs[d][0], -1))
        assert val == f'n{t}_{m}' and offs == (t,)
        assert [(k, o) for k, _, _, o in jac] == [(m, t)] and jac[0][2] in ('(T)1', '(T)1.0')
    mixed = Mixed((0, 1))
    kind, prog = lbm.link_form(mixed, lbm.AdjointBoundaryCondition(mixed), view)
    assert kind == 'neighbour'
    d = dirs.index((1, -1))
    t, m = dirs.index((1, 0)), dirs.index((-1, -1))
    lines, val, jac, offs = prog[d]
    assert offs == (t,) and sorted((k, o) for k, _, _, o in jac) == [(0, 0), (m, t)]
    # the Jacobian read off a user adjoint object's assignments is the derived one

    class Parsed(lbm.AdjointBoundaryCondition):
        pass
    parsed = lbm.neighbour_link_program(mixed, Parsed(mixed), view)
    env = {'c0': 0.4, f'n{t}_{m}': 0.03}

    def ev(e):
        return eval(e.replace('(T)', ''), {}, dict(env))
    got = {(k, o): ev(e) for k, _, e, o in parsed[d][2]}
    assert got == pytest.approx({(k, o): ev(e) for k, _, e, o in jac}, rel=1e-14)
    assert got[(m, t)] == pytest.approx(1 + 0.1 * 0.4) and got[(0, 0)] == pytest.approx(0.1 * 0.03)
    # own-cell programs keep their (lines, value, ((k, lines_k, J), …)) tuples
    fd = lbm.FixedDensity(1.01)
    kind, prog = lbm.link_form(fd, lbm.AdjointBoundaryCondition(fd), view)
    assert kind == 'program' and all(len(row) == 3 and all(len(r) == 3 for r in row[2]) for row in prog[1:])

    class Far(lbm.NeighbourBoundary):
        def __call__(self, pdf_field, direction, lb_method, **kw):
            c = dirs[direction]
            return [ps.Assignment(pdf_field[c](st.inverse_direction_index(direction)), pdf_field[2, 0](direction))]
    with pytest.raises(NotImplementedError, match=r'\(2, 0\)'):
        lbm.link_form(Far(), lbm.AdjointBoundaryCondition(Far()), view)

    class Remote(lbm.Boundary):
        def __call__(self, pdf_field, direction, lb_method, **kw):
            c = dirs[direction]
            return [ps.Assignment(pdf_field[c](st.inverse_direction_index(direction)), pdf_field[1, 0](direction))]
    with pytest.raises(NotImplementedError, match='NeighbourBoundary'):
        lbm.link_form(Remote(), lbm.AdjointBoundaryCondition(Remote()), view)
    step = lbm.AutoDiffLatticeBoltzmannStep(lbm.create_lb_update_rule('D2Q9', compressible=True), domain_size=(6, 5),
                                            relaxation_rate=1.0, target='cpu')
    with pytest.raises(NotImplementedError):
        step.set_boundary_including_adjoint(Remote())
    with pytest.raises(NotImplementedError):
        step.set_boundary_including_adjoint(Far())
    step.set_boundary_including_adjoint(mixed, lbm.make_slice[:, 0])


def test_fix_cells_cover_sources_and_targets():
    """The fix-up list of the HIP adjoint: every fluid cell next to a neighbour-link wall and every fluid cell such a
    link reads (here the row next to an outflow plane and the row one step further in)."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import fix_cells
    step, *_ = _lattice('outflow2', 'D2Q9', (6, 7), 'cpu')
    progs = step._programs()
    cells = fix_cells(step.boundary_handling.flags, step.method, [k for k, p in enumerate(progs) if p], progs)
    want = np.zeros((6, 7), bool)
    want[:, [1, 2, 4, 5]] = True
    assert np.array_equal(cells, want)
    step, *_ = _lattice('slip', 'D2Q9', (6, 7), 'cpu')
    progs = step._programs()
    cells = fix_cells(step.boundary_handling.flags, step.method, [k for k, p in enumerate(progs) if p], progs)
    want[:] = False
    want[:, [1, 5]] = True
    assert np.array_equal(cells, want)


# --- T steps and their adjoint, C kernels ------------------------------------------------------------------------
CPU_CASES = [('slip', 'D2Q9', (12, 9), 'srt', True),        # the tangential read wraps around axis 0
             ('slip', 'D2Q9', (9, 5), 'srt', True),         # a channel three cells wide
             ('outflow2', 'D2Q9', (9, 5), 'srt', True),     # ... its middle row read from both sides
             ('box', 'D2Q9', (10, 8), 'srt', True),         # the fallback at the corners, two links on one entry
             ('open', 'D2Q9', (16, 9), 'srt', True),        # own-cell programs and neighbour links together
             ('slip', 'D3Q19', (9, 6, 5), 'srt', True),
             ('box', 'D2Q9', (10, 8), 'trt', False),
             ('open', 'D2Q9', (12, 9), 'mrt', True),
             ('mixed', 'D2Q9', (7, 6), 'srt', True)]        # Jacobians that read the neighbour


@pytest.mark.parametrize('name,stencil,shape,method,compressible', CPU_CASES)
def test_neighbour_links_cpu(name, stencil, shape, method, compressible, monkeypatch):
    """T = 5 steps and their adjoint on the C lattice kernels (more than one OpenMP thread: the second adjoint pass
    adds into other cells) vs the restatement: 1e-13 forward, 1e-12 adjoint, relative to the array's max."""
    monkeypatch.setenv('OMP_NUM_THREADS', '4')          # (read when the OpenMP runtime starts; if it has, set it there)
    try:
        import ctypes
        ctypes.CDLL('libgomp.so.1').omp_set_num_threads(4)
    except (OSError, AttributeError):
        pass
    T = 5
    step, kinds, w_odd, mrt = _lattice(name, stencil, shape, 'cpu', method=method, compressible=compressible)
    ids = step.boundary_handling.flags
    f0, g, ref, gref = _reference(name, stencil, shape, method, compressible, T, kinds, ids, w_odd, mrt)
    K = step._lattice_kernels()
    assert K.programs is not None and K.link_pass
    step.set_pdfs(f0)
    step.run(T, record=True)
    err = np.abs(step.pdf_array - ref).max() / np.abs(f0).max()
    step.set_adjoint_pdfs(g)
    step.run_backward(T)
    gerr = np.abs(step.adjoint_pdf_array - gref).max() / np.abs(gref).max()
    print(f'{name} {stencil} {shape} {method}: forward {err:.2e}, adjoint {gerr:.2e}')
    assert err <= 1e-13
    assert gerr <= 1e-12


def _uniform_flow(shape, u_t):
    vel = np.zeros(shape + (len(shape),))
    vel[..., 0] = u_t
    return OL.equilibrium(np.ones(shape), vel, 'D2Q9' if len(shape) == 2 else 'D3Q19', True)


@pytest.mark.parametrize('stencil,shape', [('D2Q9', (12, 9)), ('D3Q19', (7, 6, 5))])
def test_free_slip_keeps_tangential_flow(stencil, shape):
    """Between flat free-slip walls a uniform tangential equilibrium flow is a fixed point of the step (drift after 50
    steps at most 1e-13) and the fluid cells' mass is conserved (1e-13); between no-slip walls the same flow decays
    (drift above 1e-3)."""
    drift = {}
    for wall in ('slip', 'noslip'):
        if wall == 'slip':
            step, *_ = _lattice('slip', stencil, shape, 'cpu')
        else:
            rule = lbm.create_lb_update_rule(stencil, compressible=True)
            step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=OMEGA, target='cpu')
            for end in (0, -1):
                step.set_boundary_including_adjoint(lbm.NoSlip(), _end(len(shape), 1, end))
        fluid = step.boundary_handling.flags == 0
        f0 = _uniform_flow(shape, 0.05)
        step.set_pdfs(f0)
        step.run(50)
        f = np.asarray(step.pdf_array)
        drift[wall] = np.abs(f - f0)[fluid].max()
        if wall == 'slip':
            assert abs(f[fluid].sum() - f0[fluid].sum()) <= 1e-13 * f0[fluid].sum()
    print(f'{stencil} {shape}: drift free-slip {drift["slip"]:.2e}, no-slip {drift["noslip"]:.2e}')
    assert drift['slip'] <= 1e-13
    assert drift['noslip'] > 1e-3


# --- the source of the lattices the kernels took before ----------------------------------------------------------
def _existing_lattices():
    """name → a kernel builder (target) for lattices without neighbour links: no walls, no-slip, UBB plain and
    density-weighted, FixedDensity, forces; SRT, TRT and MRT."""
    def walls(step, D, kind):
        def sl(ax, end):
            s = [slice(None)] * D
            s[ax] = end
            return tuple(s)
        if kind == 'noslip':
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl(1, 0))
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl(1, -1))
        elif kind in ('ubb', 'ubb_rho'):
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl(1, 0))
            step.set_boundary_including_adjoint(
                lbm.UBB((0.05,) + (0.0,) * (D - 1), density_weighted=kind == 'ubb_rho'), sl(1, -1))
        elif kind == 'pressure':
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl(1, 0))
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl(1, -1))
            inner = tuple(slice(1, -1) if a == 1 else slice(None) for a in range(1, D))
            step.set_boundary_including_adjoint(lbm.FixedDensity(1.02, name='inlet'), (0,) + inner)
            step.set_boundary_including_adjoint(lbm.FixedDensity(0.98, name='outlet'), (-1,) + inner)
    om = sp.Symbol('omega')
    cases = []
    for stencil in ('D2Q9', 'D3Q19'):
        D = 2 if stencil == 'D2Q9' else 3
        for comp in (True, False):
            for wk in (None, 'noslip', 'ubb', 'ubb_rho', 'pressure'):
                cases.append((f'{stencil}-{"c" if comp else "i"}-srt-{wk}-float64', stencil, D,
                              dict(compressible=comp), wk))
        cases.append((f'{stencil}-c-srt-pressure-float32', stencil, D, dict(compressible=True, data_type='float32'),
                      'pressure'))
        cases.append((f'{stencil}-c-srt-None-float32', stencil, D, dict(compressible=True, data_type='float32'), None))
        for wk in (None, 'noslip', 'pressure'):
            cases.append((f'{stencil}-c-trt-{wk}', stencil, D, dict(compressible=True, method='trt'), wk))
            cases.append((f'{stencil}-c-mrt-{wk}', stencil, D,
                          dict(compressible=True, method='mrt', relaxation_rates=[om, 1.1, 0.9, 1.2]), wk))
        for fm in ('simple', 'guo'):
            F = tuple(1e-3 * (a + 1) for a in range(D))
            cases.append((f'{stencil}-c-srt-noslip-{fm}', stencil, D,
                          dict(compressible=True, force_model=fm, force=F), 'noslip'))
            cases.append((f'{stencil}-i-srt-None-{fm}-field', stencil, D,
                          dict(compressible=False, force_model=fm, force='field'), None))
    cases.append(('D3Q27-c-srt-noslip-float64', 'D3Q27', 3, dict(compressible=True), 'noslip'))
    out = {}
    for name, stencil, D, kw, wk in cases:
        def build(target, stencil=stencil, D=D, kw=kw, wk=wk):
            kw = dict(kw)
            if kw.get('force') == 'field':
                kw['force'] = ps.fields(f'F({D}): float64[{D}D]')
            rule = lbm.create_lb_update_rule(stencil, **kw)
            step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(8, 6, 5)[:D], relaxation_rate=1.3,
                                                    target=target)
            if wk is not None:
                walls(step, D, wk)
            assert step._lattice is not None
            return step._lattice_kernels()
        out[name] = build
    return out


def _source_shas():
    """sha256 of every emitted source of those lattices: the C target, and the HIP main (and, with link programs,
    fix-up) modules in both addressing modes. Nothing is compiled."""
    shas = {}
    for name, build in _existing_lattices().items():
        K = build('cpu')
        shas[f'{name}/c'] = hashlib.sha256(K.source().encode()).hexdigest()
        K = build('gpu')
        for addr in ('buf', 'ptr'):
            shas[f'{name}/hip-{addr}'] = hashlib.sha256(K.source('int', addr).encode()).hexdigest()
            if K.programs is not None:
                shas[f'{name}/hip-{addr}-fix'] = hashlib.sha256(K.source('int', addr, fix=True).encode()).hexdigest()
    return shas


def test_existing_lattice_sources_unchanged():
    """The emitted kernel source of every lattice without neighbour links is byte-identical to what it was before
    they existed (``tests/golden/lattice_source_sha.json``, generated at that commit by ``_source_shas``)."""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    shas = _source_shas()
    assert sorted(shas) == sorted(golden)
    assert [k for k in golden if shas[k] != golden[k]] == []


def _all_lattices():
    """name → a kernel builder (target) of every lattice whose sources ``lattice_source_sha_all.json`` pins: the
    lattices above, the compile-test families of ``test_lbm_addressing``, the neighbour-link lattices, and one
    lattice per branch of the source printer that none of those reaches."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    from tests import test_lbm_addressing as TA
    out = dict(_existing_lattices())

    def family(make):
        def build(target):
            K = make()._lattice_kernels()          # the families build GPU steps: the C twin from the same description
            return K if target == 'gpu' else LatticeKernels(
                K.stencil, K.compressible, K.dtype, K.walls, target, K.links, K.force_model, K.force, K.force_field,
                trt=K.trt, programs=K.programs, mrt=K.mrt)
        return build
    for name, make in TA.COMPILE_FAMILIES:
        out[f'family-{name}'] = family(make)

    def neighbour(name, stencil, shape, method='srt', compressible=True):
        return lambda target: _lattice(name, stencil, shape, target, 'float64', method,
                                       compressible)[0]._lattice_kernels()
    for name in ('slip', 'mixed', 'outflow2', 'box', 'open'):
        out[f'nb-{name}-D2Q9'] = neighbour(name, 'D2Q9', (8, 6))
    for name in ('slip', 'box'):
        out[f'nb-{name}-D3Q19'] = neighbour(name, 'D3Q19', (8, 6, 5))
    for method in ('trt', 'mrt'):
        out[f'nb-open-D2Q9-{method}'] = neighbour('open', 'D2Q9', (8, 6), method)
    out['nb-open-D2Q9-incompressible'] = neighbour('open', 'D2Q9', (8, 6), compressible=False)

    om = sp.Symbol('omega')
    methods = dict(srt={}, trt=dict(method='trt'), mrt=dict(method='mrt', relaxation_rates=[om, 1.1, 0.9, 1.2]),
                   trtrate=dict(method='trt', relaxation_rates=[om, 1.1]))

    def branch(method, model=None, field=False, walls=None, check=lambda K: True):
        def build(target):
            kw = dict(methods[method], compressible=True)
            if model is not None:
                kw.update(force_model=model, force=ps.fields('F(2): float64[2D]') if field else (1e-3, 2e-3))
            step = lbm.AutoDiffLatticeBoltzmannStep(lbm.create_lb_update_rule('D2Q9', **kw), domain_size=(8, 6),
                                                    relaxation_rate=1.3, target=target)
            if walls is not None:
                step.set_boundary_including_adjoint(lbm.NoSlip(), (slice(None), 0))
                step.set_boundary_including_adjoint(
                    lbm.UBB((0.05, 0.0), density_weighted=True) if walls == 'rho+pressure' else lbm.NoSlip(),
                    (slice(None), -1))
            if walls == 'rho+pressure':
                step.set_boundary_including_adjoint(lbm.FixedDensity(1.02, name='inlet'), (0, slice(1, -1)))
            assert step._lattice is not None
            K = step._lattice_kernels()
            assert check(K)
            return K
        return build
    for method in ('trt', 'mrt'):
        out[f'branch-guo-{method}'] = branch(method, 'guo')                       # gsplit, a constant force
        out[f'branch-guo-{method}-field'] = branch(method, 'guo', True)           # gsplit, a force field
        out[f'branch-simple-{method}-field'] = branch(method, 'simple', True)     # gwm
    for model in ('simple', 'guo'):
        out[f'branch-{model}-field-walls'] = branch('srt', model, True, 'noslip', lambda K: K.walls and K.force_field)
    out['branch-trt-rate'] = branch('trtrate', check=lambda K: K.trt == ('rate', 1.1))
    out['branch-trt-rate-walls'] = branch('trtrate', walls='noslip', check=lambda K: K.trt == ('rate', 1.1))
    # a density-weighted wall and a link program in one lattice: scratch slot Q on C, the single slot on HIP
    out['branch-ubb-rho-pressure'] = branch('srt', walls='rho+pressure',
                                            check=lambda K: K.rho_links and K.programs is not None)
    return out


def _all_source_shas():
    """sha256 of every emitted source of ``_all_lattices``: the C target, and the HIP main (and, with link programs,
    fix-up) modules for both index types in both addressing modes. One kernel object per target; nothing is
    compiled."""
    def sha(s):
        return hashlib.sha256(s.encode()).hexdigest()
    shas = {}
    for name, build in _all_lattices().items():
        shas[f'{name}/c'] = sha(build('cpu').source())
        K = build('gpu')
        for idx in ('int', 'long long'):
            for addr in ('buf', 'ptr'):
                for fix in ((False, True) if K.programs is not None else (False,)):
                    shas[f'{name}/hip-{idx.replace(" ", "")}-{addr}{"-fix" if fix else ""}'] = \
                        sha(K.source(idx, addr, fix=fix))
    return shas


def test_all_lattice_sources_unchanged():
    """The emitted kernel source of every lattice of ``_all_lattices``, every index type and addressing mode, is
    byte-identical to what the one-function printer gave before it was split into ``_lattice_source``
    (``tests/golden/lattice_source_sha_all.json``, generated at the commit before the split by ``_all_source_shas``)."""
    with open(GOLDEN_ALL) as fh:
        golden = json.load(fh)
    shas = _all_source_shas()
    assert sorted(shas) == sorted(golden)
    assert [k for k in golden if shas[k] != golden[k]] == []


def _declared_formats(source):
    """kernel name → the ``struct`` codes of its parameter list, parsed out of the emitted HIP text: a pointer is
    ``Q``, ``const int`` ``i``, ``const IDX`` ``i`` / ``q`` by the typedef, ``const long long`` ``q``, ``const float`` /
    ``const double`` ``f`` / ``d``."""
    import re
    idx = re.search(r'^typedef (.+) IDX;$', source, re.M).group(1)
    scalar = {'const int': 'i', 'const IDX': {'int': 'i', 'long long': 'q'}[idx], 'const long long': 'q',
              'const float': 'f', 'const double': 'd'}
    out = {}
    for name, params in re.findall(r'^extern "C" __global__ void __launch_bounds__\(\d+\) (\w+)\(([^)]*)\)$', source,
                                   re.M):
        out[name] = ''.join('Q' if '*' in p else scalar[p.strip().rsplit(' ', 1)[0]] for p in params.split(','))
    return out


def test_launch_formats_match_the_emitted_signatures():
    """The launcher's argument-buffer format of every kernel (``LatticeKernels.arg_format``) is the parameter list the
    printer emits for it: every lattice of ``_all_lattices`` plus a float16, an ω-field, a force-field and a Smagorinsky
    lattice, both index types, ``lbm_fwd`` / ``lbm_adj`` / ``lbm_adj_rho`` (lattices with a second pass on the HIP
    target) / ``lbm_adj_fix`` (lattices with link programs). Nothing is compiled."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    st = lbm.LBStencil('D3Q19')
    lattices = {name: build('gpu') for name, build in _all_lattices().items()}
    lattices['float16'] = LatticeKernels(st, True, np.float16, True, 'gpu', zero_centered=True)
    lattices['omega-field'] = LatticeKernels(st, True, np.float32, False, 'gpu', omega_field=True)
    lattices['force-field'] = LatticeKernels(st, False, np.float64, True, 'gpu', force_model='guo', force_field=True)
    lattices['smagorinsky'] = LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float64, True, 'gpu', smagorinsky=0.12,
                                             omega_field=True)
    seen = set()
    for name, K in lattices.items():
        for idx, addr in (('int', 'buf'), ('long long', 'ptr')):
            main = _declared_formats(K.source(idx, addr))
            assert sorted(main) == ['lbm_adj'] + ['lbm_adj_rho'] * bool(K.rho_links) + ['lbm_fwd'], name
            fix = _declared_formats(K.source(idx, addr, fix=True)) if K.programs is not None else {}
            assert sorted(fix) == ['lbm_adj_fix'] * (K.programs is not None), name
            for kernel, fmt in {**main, **fix}.items():
                assert K.arg_format(kernel[len('lbm_'):], idx) == fmt, (name, idx, kernel)
                seen.add(kernel)
    assert seen == {'lbm_fwd', 'lbm_adj', 'lbm_adj_rho', 'lbm_adj_fix'}


# --- HIP kernels -----------------------------------------------------------------------------------------------
GPU_CASES = [('slip', 'D2Q9', (70, 33), 'float64', 'srt', True),      # x no multiple of 64, the tangential read wraps
             ('box', 'D2Q9', (64, 40), 'float32', 'trt', False),      # the corner fallback
             ('slip', 'D2Q9', (66, 5), 'float64', 'srt', True),       # the three-cell channel
             ('open', 'D2Q9', (70, 33), 'float64', 'srt', True),      # FixedDensity inlet, outflow outlet, free-slip
             ('slip', 'D3Q19', (20, 12, 10), 'float64', 'srt', True),
             ('mixed', 'D2Q9', (34, 9), 'float64', 'srt', True)]      # Jacobians that read the neighbour


@pytest.mark.gpu
@pytest.mark.parametrize('name,stencil,shape,dtype,method,compressible', GPU_CASES)
def test_neighbour_links_gpu(name, stencil, shape, dtype, method, compressible):
    """T = 6 steps and their adjoint on the HIP lattice kernels, through ``run`` / ``run_backward`` and through the
    time-step op, vs the restatement: 1e-12 / 1e-11 (float64), 2e-5 / 2e-4 (float32), relative to the array's max."""
    import torch
    T = 6
    step, kinds, w_odd, mrt = _lattice(name, stencil, shape, 'gpu', dtype, method, compressible)
    ids = step.boundary_handling.flags
    f0, g, ref, gref = _reference(name, stencil, shape, method, compressible, T, kinds, ids, w_odd, mrt)
    tdt = getattr(torch, dtype)
    tol, gtol = (1e-12, 1e-11) if dtype == 'float64' else (2e-5, 2e-4)
    step.set_pdfs(torch.tensor(f0, dtype=tdt, device='cuda'))
    step.run(T, record=True)
    err = np.abs(step.pdf_array.double().cpu().numpy() - ref).max() / np.abs(f0).max()
    step.set_adjoint_pdfs(torch.tensor(g, dtype=tdt, device='cuda'))
    step.run_backward(T)
    gerr = np.abs(step.adjoint_pdf_array.double().cpu().numpy() - gref).max() / np.abs(gref).max()
    op = step.create_timestep_op(T)
    x = torch.tensor(f0, dtype=tdt, device='cuda', requires_grad=True)
    out = op.apply(x)
    out.backward(torch.tensor(g, dtype=tdt, device='cuda'))
    err_op = np.abs(out.detach().double().cpu().numpy() - ref).max() / np.abs(f0).max()
    gerr_op = np.abs(x.grad.double().cpu().numpy() - gref).max() / np.abs(gref).max()
    print(f'{name} {stencil} {shape} {dtype}: forward {err:.2e} / op {err_op:.2e}, adjoint {gerr:.2e} / op {gerr_op:.2e}')
    assert err <= tol and err_op <= tol
    assert gerr <= gtol and gerr_op <= gtol


@pytest.mark.gpu
def test_neighbour_links_adjoint_bitwise_repeatable_gpu():
    """The flat free-slip channel puts at most two addends on an entry, so the HIP adjoint's atomic sums do not depend
    on their order: two runs give bitwise equal results."""
    import torch
    T, shape = 6, (70, 33)
    step, *_ = _lattice('slip', 'D2Q9', shape, 'gpu')
    f0 = torch.tensor(_init('D2Q9', shape, True, seed=51), device='cuda')
    g = torch.tensor(np.random.default_rng(52).standard_normal(f0.shape), device='cuda')
    res = []
    for _ in range(2):
        step.set_pdfs(f0)
        step.run(T, record=True)
        step.set_adjoint_pdfs(g)
        step.run_backward(T)
        res.append(step.adjoint_pdf_array.clone())
    assert torch.equal(res[0], res[1])
