"""The momentum-exchange force on a boundary object: ``step.create_boundary_force_op(boundary)`` and
``create_timestep_op(T, boundary_force_outputs=…)``.

The definition, restated here independently of the package ("Boundary force"): for a state ``s``
(post-collision pdfs) and the boundary object with flag id ``b``, the links are the pairs (x, d) with ``flags[x] == 0``,
``c_d ≠ 0`` and ``flags[(x + c_d) mod N] == b``, and

    F = Σ_links c_d·(f_d(x) + f_in),   f_in = α·f_d(x) + β,   f_d(x) = s_d(x) (+ w_d for zero-centred storage)

with (α, β) = (1, 0) for ``NoSlip`` and (1, −6 w_d c_d·u) for ``UBB(u)``, written out by hand in ``_reference`` (plain
numpy float64 loops over cells and directions; the sums by ``math.fsum``, so the reference's own summation error does
not enter the bound).

Bounds. The kernels accumulate in float64 whatever the storage type, so with n links
``|ΔF_a| ≤ eps(compute type)·|F_a| + (n + 4)·2⁻⁵³·Σ_links|terms_a|``: one rounding of the result to the compute type,
n − 1 float64 additions, and the few float64 roundings inside a term. Gradient: ``(1 + α)·Σ_a c_{d,a}·dF_a`` on the
links, at most three terms added in float64 (two additions: ``2·2⁻⁵³·(1 + α)·Σ_a|c_{d,a} dF_a|``) and one rounding to the
array's type (``eps(array type)·|value|``); exactly 0 off the links."""
import math

import numpy as np
import pytest

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm, ps
from tests.test_lbm import _init

OMEGA = 1.7
UBB_U = {2: (0.05, -0.02), 3: (0.04, -0.02, 0.01)}
SHAPES = {'D2Q9': (12, 10), 'D3Q19': (6, 7, 8), 'D3Q27': (5, 6, 7)}
EPS = {'float64': 2.0 ** -52, 'float32': 2.0 ** -23, 'float16': 2.0 ** -10}


def _ctype(dtype):
    return 'float64' if dtype == 'float64' else 'float32'


# --- lattices --------------------------------------------------------------------------------------------------
def _masks(shape):
    """``body``: a block touching the domain's edge along axis 0 (wrapped links) and a one-cell-thick plate one fluid
    cell away from it (the cells between have walls on two sides; the plate has fluid on both); ``lid``: the last
    layer of the last axis."""
    D = len(shape)
    body, lid = np.zeros(shape, bool), np.zeros(shape, bool)
    lo = shape[1] // 3
    if D == 2:
        body[0:2, lo:lo + 3] = True
        body[3, 1:shape[1] - 3] = True
    else:
        l2 = shape[2] // 3
        body[0:2, lo:lo + 3, l2:l2 + 2] = True
        body[3, 1:shape[1] - 3, 2:shape[2] - 2] = True
    lid[..., -1] = True
    assert not (body & lid).any()
    return body, lid


def _rule(stencil, dtype, zc=False, field=None):
    D = len(SHAPES[stencil])
    kw = {}
    if field == 'omega':
        kw['relaxation_rate'] = ps.fields(f'omega_f: {dtype}[{D}D]').center
    if field == 'sigma':
        kw['solid_fraction'] = ps.fields(f'sigma: {dtype}[{D}D]').center
    return lbm.create_lb_update_rule(stencil, compressible=True, data_type=dtype, zero_centered=zc, **kw)


def _make(stencil, shape, dtype='float64', zc=False, target='cpu', field=None, bodies=True):
    """A step with the NoSlip ``body`` and the UBB ``lid`` of ``_masks`` (two boundary objects: whichever is selected,
    the other is set but not selected)."""
    step = lbm.AutoDiffLatticeBoltzmannStep(_rule(stencil, dtype, zc, field), domain_size=shape, target=target,
                                            relaxation_rate=None if field == 'omega' else OMEGA)
    assert step._lattice is not None
    body, lid = lbm.NoSlip('body'), lbm.UBB(UBB_U[len(shape)], name='lid')
    if bodies:
        mb, ml = _masks(shape)
        step.set_boundary_including_adjoint(body, mask_array=mb)
        step.set_boundary_including_adjoint(lid, mask_array=ml)
    return step, body, lid


_STEPS = {}


def _shared(stencil, dtype='float64', zc=False, target='cpu', shape=None):
    """Steps of tests that do not change the flags, made once."""
    key = (stencil, dtype, zc, target, shape)
    if key not in _STEPS:
        _STEPS[key] = _make(stencil, shape or SHAPES[stencil], dtype, zc, target)
    return _STEPS[key]


def _weights(stencil):
    return np.array([float(v) for v in OL.SETS[stencil][1]])


def _state(stencil, shape, dtype, zc, seed=3):
    """A stored state (numpy, the pdf dtype) near an equilibrium, and what it stands for in float64."""
    f = _init(stencil, shape, True, seed=seed)
    s = (f - _weights(stencil) if zc else f).astype(dtype)
    return s


# --- the reference ---------------------------------------------------------------------------------------------
def _reference(stencil, flags, b, s, zc, u=None):
    """``F [D]``, ``Σ|terms| [D]``, the link count and the coefficient array ``∂F_a/∂s_d(x)`` ``[*domain, Q, D]`` of
    the boundary with flag id ``b`` (``u``: None for NoSlip, the wall velocity for UBB) on the stored state ``s``."""
    dirs, w = OL.SETS[stencil]
    shape, D = flags.shape, flags.ndim
    terms = [[] for _ in range(D)]
    coef = np.zeros(shape + (len(dirs), D))
    n = 0
    for x in np.ndindex(*shape):
        if flags[x] != 0:
            continue
        for d, c in enumerate(dirs):
            if not any(c) or flags[tuple((xi + ci) % ni for xi, ci, ni in zip(x, c, shape))] != b:
                continue
            wd = float(w[d])
            f = float(s[x + (d,)]) + (wd if zc else 0.0)
            alpha, beta = 1.0, 0.0 if u is None else -6.0 * wd * sum(ci * ui for ci, ui in zip(c, u))
            f_in = alpha * f + beta
            for a in range(D):
                terms[a].append(c[a] * (f + f_in))
            coef[x + (d,)] = (1.0 + alpha) * np.array(c, float)
            n += 1
    F = np.array([math.fsum(t) for t in terms])
    A = np.array([math.fsum(abs(v) for v in t) for t in terms])
    return F, A, n, coef


def _bound(F, A, n, ctype):
    return EPS[ctype] * np.abs(F) + (n + 4) * 2.0 ** -53 * A


def _apply(step, boundary, s, grad=None, cap=None):
    """The force op on the stored state ``s`` (numpy): the force and, with ``grad`` (dF), the gradient, as float64."""
    import torch
    dev = 'cuda' if step._gpu else 'cpu'
    x = torch.tensor(s, device=dev, requires_grad=grad is not None)
    F = step.create_boundary_force_op(boundary, block_cap=cap).apply(x)
    ct = torch.float64 if s.dtype == np.float64 else torch.float32
    assert F.dtype == ct and tuple(F.shape) == (s.ndim - 1,) and F.device == x.device
    if grad is None:
        return F.detach().double().cpu().numpy()
    F.backward(torch.tensor(grad, dtype=ct, device=dev))
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    return F.detach().double().cpu().numpy(), x.grad.double().cpu().numpy()


FORCE_CASES = [(st, kind, dt, zc) for st in ('D2Q9', 'D3Q19') for kind in ('noslip', 'ubb')
               for dt in ('float64', 'float32', 'float16') for zc in (False, True)] + [('D3Q27', 'ubb', 'float64', False)]


def _force_case(stencil, kind, dtype, zc, target, report=''):
    shape = SHAPES[stencil]
    step, body, lid = _shared(stencil, dtype, zc, target)
    flags = step.boundary_handling.flags
    sel, u = (body, None) if kind == 'noslip' else (lid, UBB_U[len(shape)])
    s = _state(stencil, shape, dtype, zc)
    F, A, n, _ = _reference(stencil, flags, step.boundary_handling.conditions[sel], s, zc, u)
    links = step.boundary_links(sel)
    assert links.n == n > 0 and links.cells.dtype == np.int32 and links.directions.dtype == np.uint8
    # (sorted by (direction, cell), every pair once)
    order = links.directions.astype(np.int64) * flags.size + links.cells
    assert (np.diff(order) > 0).all()
    got = _apply(step, sel, s)
    bound = _bound(F, A, n, _ctype(dtype))
    print(f'{report}{stencil} {kind} {dtype} zc={zc}: {n} links, F {F}, error {np.abs(got - F)}, bound {bound}')
    assert (np.abs(got - F) <= bound).all()
    assert np.abs(F).max() > 100 * bound.max()          # (the comparison sees the force, not only its bound)
    return got, bound


def _backward_case(stencil, kind, dtype, zc, target):
    shape = SHAPES[stencil]
    D = len(shape)
    step, body, lid = _shared(stencil, dtype, zc, target)
    flags = step.boundary_handling.flags
    sel, u = (body, None) if kind == 'noslip' else (lid, UBB_U[D])
    s = _state(stencil, shape, dtype, zc)
    _, _, n, coef = _reference(stencil, flags, step.boundary_handling.conditions[sel], s, zc, u)
    dF = np.array([0.7, -1.3, 0.45][:D]).astype(_ctype(dtype)).astype(np.float64)
    _, g = _apply(step, sel, s, grad=dF)
    ref = (coef * dF).sum(-1)
    on = np.abs(coef).sum(-1) > 0
    assert int(on.sum()) == n
    assert (g[~on] == 0).all()
    bound = EPS[dtype] * np.abs(ref) + 2 * 2.0 ** -53 * (np.abs(coef) * np.abs(dF)).sum(-1)
    print(f'{stencil} {kind} {dtype}: gradient error {np.abs(g - ref).max():.3e}, bound at that entry '
          f'{bound.flat[np.abs(g - ref).argmax()]:.3e}')
    assert (np.abs(g - ref) <= bound).all() and np.abs(ref[on]).min() > 0
    return g


# --- CPU target ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stencil,kind,dtype,zc', FORCE_CASES)
def test_force_cpu_vs_reference(stencil, kind, dtype, zc):
    _force_case(stencil, kind, dtype, zc, 'cpu')


@pytest.mark.parametrize('stencil', ['D2Q9', 'D3Q19'])
@pytest.mark.parametrize('dtype', ['float64', 'float32', 'float16'])
def test_flat_wall_and_closed_block_known_answers(stencil, dtype):
    """Uniform ``f = w·ρ0`` at rest. A flat NoSlip wall across the periodic box with fluid on one side (another
    boundary object lies against its other side): the pressure ρ0/3 per unit area, along the direction from the fluid
    into the wall (D2Q9: 2·(1/9 + 2/36) = 1/3 per wall cell). A closed block: 0."""
    shape = SHAPES[stencil]
    D, rho0 = len(shape), 1.25
    step, _, _ = _make(stencil, shape, dtype, bodies=False)
    wall, back, block = lbm.NoSlip('wall'), lbm.NoSlip('back'), lbm.NoSlip('block')
    last = (slice(None),) * (D - 1)
    step.set_boundary_including_adjoint(wall, last + (0,))
    step.set_boundary_including_adjoint(back, last + (-1,))          # (periodic: the wall's other side)
    mb = np.zeros(shape, bool)
    mb[(slice(2, 4),) * (D - 1) + (slice(3, 5),)] = True
    step.set_boundary_including_adjoint(block, mask_array=mb)
    s = np.broadcast_to(_weights(stencil) * rho0, shape + (len(_weights(stencil)),)).astype(dtype)
    area = int(np.prod(shape[:-1]))
    for sel, want in ((wall, np.array([0.0] * (D - 1) + [-rho0 / 3 * area])), (block, np.zeros(D))):
        F, A, n, _ = _reference(stencil, step.boundary_handling.flags, step.boundary_handling.conditions[sel], s, False)
        got = _apply(step, sel, s)
        # (the stored weights are rounded to the pdf dtype: the known answer holds to that rounding of the inputs)
        slack = (0 if dtype == 'float64' else EPS[dtype] / 2) * A
        bound = _bound(want, A, n, _ctype(dtype)) + slack
        print(f'{stencil} {dtype} {sel.name}: {got} against {want}, bound {bound}')
        assert (np.abs(got - want) <= bound).all() and (np.abs(got - F) <= _bound(F, A, n, _ctype(dtype))).all()


@pytest.mark.parametrize('stencil', ['D2Q9', 'D3Q19'])
def test_momentum_balance_with_the_time_step(stencil):
    """One time step of the package (float64, no body force) on the lattice with the NoSlip body and the UBB lid:
    the fluid's momentum changes by minus the forces on all boundaries,
    ``Σ_fluid Σ_i c_i (s'_i − s_i) = −Σ_B F_B(s)``, to ``(Q·cells + n_links)·2⁻⁵³·Σ|terms|``."""
    import torch
    shape = SHAPES[stencil]
    step, body, lid = _shared(stencil)
    flags = step.boundary_handling.flags
    s = _state(stencil, shape, 'float64', False, seed=8)
    s1 = step.create_timestep_op(1).apply(torch.tensor(s)).numpy()
    c = np.array(OL.SETS[stencil][0], float)                # [Q, D]
    fluid = flags == 0
    change = ((s1 - s)[fluid] @ c).sum(0)
    mag = (np.abs(s1[fluid]) @ np.abs(c)).sum(0) + (np.abs(s[fluid]) @ np.abs(c)).sum(0)
    total, nl = np.zeros(len(shape)), 0
    for sel, u in ((body, None), (lid, UBB_U[len(shape)])):
        F = _apply(step, sel, s)
        _, A, n, _ = _reference(stencil, flags, step.boundary_handling.conditions[sel], s, False, u)
        total, mag, nl = total + F, mag + A, nl + n
    bound = (c.shape[0] * flags.size + nl) * 2.0 ** -53 * mag
    print(f'{stencil}: momentum change {change}, forces {total}, residual {np.abs(change + total)}, bound {bound}')
    assert (np.abs(change + total) <= bound).all() and np.abs(total).max() > 1e6 * bound.max()


@pytest.mark.parametrize('stencil,kind,dtype', [('D2Q9', 'noslip', 'float64'), ('D2Q9', 'ubb', 'float32'),
                                                ('D2Q9', 'noslip', 'float16'), ('D3Q19', 'ubb', 'float64'),
                                                ('D3Q19', 'noslip', 'float32'), ('D3Q27', 'noslip', 'float64'),
                                                ('D3Q27', 'ubb', 'float32')])
def test_backward_cpu_is_the_coefficient_array(stencil, kind, dtype):
    _backward_case(stencil, kind, dtype, False, 'cpu')


def test_gradcheck_float64():
    import torch
    shape = (5, 4)
    step, _, _ = _make('D2Q9', shape, bodies=False)
    body = lbm.UBB((0.03, 0.02), name='body')
    mb = np.zeros(shape, bool)
    mb[2, 1:3] = True
    step.set_boundary_including_adjoint(body, mask_array=mb)
    x = torch.tensor(_state('D2Q9', shape, 'float64', False), requires_grad=True)
    assert torch.autograd.gradcheck(step.create_boundary_force_op(body).apply, (x,))


# --- the time-step op ------------------------------------------------------------------------------------------
def _timestep_inputs(step, shape, field, dtype='float64', dev='cpu', seed=21):
    import torch
    rng = np.random.default_rng(seed)
    tdt = getattr(torch, dtype)
    x = torch.tensor(_init('D2Q9' if len(shape) == 2 else 'D3Q19', shape, True, seed=seed), dtype=tdt, device=dev,
                     requires_grad=True)
    extras = []
    if field == 'omega':
        extras = [torch.tensor(OMEGA + 0.1 * rng.random(shape), dtype=tdt, device=dev, requires_grad=True)]
    if field == 'sigma':
        extras = [torch.tensor(0.3 * rng.random(shape), dtype=tdt, device=dev, requires_grad=True)]
    return x, extras, rng


def _chain(step, specs, x, extras, T, macro):
    """T one-step ops with the force op applied between them by autograd: (pdfs, [rho, vel,] force…) as the T-step op
    returns them (``macro``: None or the k of ``macroscopic_outputs``)."""
    import torch
    one = step.create_timestep_op(1, macroscopic_outputs=None if macro is None else 1)
    fops = [step.create_boundary_force_op(b) for b, _ in specs]
    f, forces, rho, vel = x, [[] for _ in specs], [], []
    for t in range(1, T + 1):
        if macro is None:
            f = one.apply(f, *extras)
        else:
            f, r, v = one.apply(f, *extras)
            if t % macro == 0:
                rho.append(r[0])
                vel.append(v[0])
        for i, (_, k) in enumerate(specs):
            if t % k == 0:
                forces[i].append(fops[i].apply(f))
    out = [f] + ([torch.stack(rho), torch.stack(vel)] if macro is not None else [])
    return out + [torch.stack(fs) for fs in forces]


def _weighted(outs, seeds):
    return sum((o * w).sum() for o, w in zip(outs, seeds) if w is not None)


@pytest.mark.parametrize('field', [None, 'omega', 'sigma'])
@pytest.mark.parametrize('macro', [False, True], ids=['plain', 'macroscopic'])
@pytest.mark.parametrize('k', [1, 2])
def test_timestep_op_against_the_chain_of_one_step_ops(k, macro, field):
    """T = 5, float64, the C kernels: forces at 1e-13 and every gradient at 1e-12 of the maximum (the bounds of
    ``test_lbm_macroscopic_outputs``' CPU comparison); the body's force every k steps and the lid's every step."""
    import torch
    shape, T = SHAPES['D2Q9'], 5
    step, body, lid = _make('D2Q9', shape, field=field)
    specs = [(body, k), (lid, 1)]
    x, extras, rng = _timestep_inputs(step, shape, field)
    op = step.create_timestep_op(T, macroscopic_outputs=k if macro else None,
                                 boundary_force_outputs=[(body, k), lid])
    assert op.boundary_force_states == (tuple(range(k, T + 1, k)), (1, 2, 3, 4, 5))
    outs = op.apply(x, *extras)
    assert len(outs) == (5 if macro else 3) and tuple(outs[-2].shape) == (T // k, 2) and tuple(outs[-1].shape) == (T, 2)
    seeds = [torch.tensor(rng.standard_normal(tuple(o.shape))) for o in outs]
    ins = [x] + extras
    got = torch.autograd.grad(_weighted(outs, seeds), ins)
    ref_outs = _chain(step, specs, x, extras, T, k if macro else None)
    ref = torch.autograd.grad(_weighted(ref_outs, seeds), ins)
    for what, a, b, tol in [('out', o, r, 1e-13) for o, r in zip(outs, ref_outs)] + \
            [('grad', g, r, 1e-12) for g, r in zip(got, ref)]:
        err, scale = float((a.detach() - b.detach()).abs().max()), float(b.detach().abs().max())
        print(f'{what} {tuple(a.shape)}: error {err:.3e} of {scale:.3e}')
        assert scale > 0 and err <= tol * scale
    # (the force seeds matter: without them the gradient is another)
    plain = torch.autograd.grad(_weighted(op.apply(x, *extras)[:1], seeds[:1]), ins)
    assert float((plain[0] - got[0]).abs().max()) > 1e-3 * float(got[0].abs().max())


def test_single_boundary_spec_and_observables_only():
    """``boundary_force_outputs=body`` (no list, k = 1); a loss on the forces alone (the pdf gradient None)."""
    import torch
    shape, T = SHAPES['D2Q9'], 3
    step, body, lid = _make('D2Q9', shape)
    x, extras, rng = _timestep_inputs(step, shape, None)
    out, F = step.create_timestep_op(T, boundary_force_outputs=body).apply(x)
    assert tuple(F.shape) == (T, 2)
    seed = torch.tensor(rng.standard_normal((T, 2)))
    (got,) = torch.autograd.grad((F * seed).sum(), x)
    ref_outs = _chain(step, [(body, 1)], x, extras, T, None)
    (ref,) = torch.autograd.grad((ref_outs[1] * seed).sum(), x)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='boundary_force_outputs'):
            step.create_timestep_op(T, boundary_force_outputs=(body, bad))


def test_none_is_the_plain_op_and_grad_is_not_modified():
    """``boundary_force_outputs=None``: bitwise the op without the keyword (outputs and gradients); the observed op's
    pdfs and, with force gradients None, its gradient are bitwise the plain op's; a ``grad`` that is the caller's
    tensor is not modified when the force of the last state is seeded."""
    import torch
    shape, T = SHAPES['D2Q9'], 5
    step, body, lid = _make('D2Q9', shape)
    x, _, rng = _timestep_inputs(step, shape, None)
    c = torch.tensor(rng.standard_normal(shape + (9,)))
    res = {}
    for name, kw in (('default', {}), ('none', dict(boundary_force_outputs=None)),
                     ('observed', dict(boundary_force_outputs=body))):
        out = step.create_timestep_op(T, **kw).apply(x)
        out = out[0] if name == 'observed' else out
        assert torch.is_tensor(out)
        res[name] = (out.detach().clone(), torch.autograd.grad((out * c).sum(), x)[0])
    for name in ('none', 'observed'):
        assert torch.equal(res['default'][0], res[name][0]) and torch.equal(res['default'][1], res[name][1])
    out, F = step.create_timestep_op(T, boundary_force_outputs=body).apply(x)
    keep = c.clone()
    (seeded,) = torch.autograd.grad([out, F], x, [c, torch.ones_like(F)])
    assert torch.equal(c, keep)
    assert not torch.equal(seeded, res['default'][1])


def test_end_to_end_boundary_force_trajectory():
    import torch
    shape = SHAPES['D2Q9']
    step, body, lid = _make('D2Q9', shape)
    rng = np.random.default_rng(1)
    rho = torch.tensor(1 + 0.01 * rng.standard_normal(shape))
    vel = torch.tensor(0.03 * rng.standard_normal(shape + (2,)), requires_grad=True)
    r = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1, boundary_force_outputs=body)
    plain = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1)
    assert not hasattr(plain, 'boundary_force_trajectory') and tuple(r.boundary_force_trajectory.shape) == (2, 2)
    assert torch.equal(r.output_pdf_tensor, plain.output_pdf_tensor)
    F = step.create_boundary_force_op(body).apply(plain.output_pdf_tensor)
    assert torch.equal(F, r.boundary_force_trajectory[1])
    (g,) = torch.autograd.grad(r.boundary_force_trajectory.sum(), vel)
    assert float(g.abs().max()) > 0
    # the time-step op's spellings: a (boundary, 1) pair is the boundary; a list gives a list; another k is refused
    pair = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1, boundary_force_outputs=(body, 1))
    assert torch.equal(pair.boundary_force_trajectory, r.boundary_force_trajectory)
    both = step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1, boundary_force_outputs=[body, lid])
    assert len(both.boundary_force_trajectory) == 2 and torch.equal(both.boundary_force_trajectory[0],
                                                                    r.boundary_force_trajectory)
    with pytest.raises(ValueError, match='pairs'):
        step.create_end_to_end_op(4, vel, rho, num_times_steps_without_save=1, boundary_force_outputs=(body, 2))


# --- refusals and edge cases -----------------------------------------------------------------------------------
def test_refusals_name_the_boundary():
    shape = SHAPES['D2Q9']
    step, body, lid = _make('D2Q9', shape, bodies=False)
    cases = [lbm.FixedDensity(1.01, name='inlet'), lbm.FreeSlip((0, 1), name='slip'),
             lbm.ZeroGradientOutflow((0, -1), name='outflow'), lbm.UBB((0.01, 0.0), name='heavy', density_weighted=True)]
    for i, b in enumerate(cases):
        step.set_boundary_including_adjoint(b, lbm.make_slice[2 * i, 2:5])
        for make in (step.boundary_links, step.create_boundary_force_op,
                     lambda bb: step.create_timestep_op(2, boundary_force_outputs=bb)):
            with pytest.raises(NotImplementedError, match=b.name):
                make(b)
    with pytest.raises(ValueError, match='never set'):
        step.create_boundary_force_op(lbm.NoSlip('elsewhere'))
    with pytest.raises(ValueError, match='never set'):
        step.boundary_links(body)


def test_zero_link_boundaries():
    """A boundary with no fluid neighbour (enclosed by another object) and one that covers the lattice: force exactly
    0, gradient exactly 0, no error — in the force op and in the time-step op."""
    import torch
    shape = SHAPES['D2Q9']
    step, _, _ = _make('D2Q9', shape, bodies=False)
    core, shell = lbm.NoSlip('core'), lbm.NoSlip('shell')
    m = np.zeros(shape, bool)
    m[3:8, 3:8] = True
    step.set_boundary_including_adjoint(shell, mask_array=m)
    m2 = np.zeros(shape, bool)
    m2[4:7, 4:7] = True
    step.set_boundary_including_adjoint(core, mask_array=m2)
    assert step.boundary_links(core).n == 0 and step.boundary_links(shell).n > 0
    x = torch.tensor(_state('D2Q9', shape, 'float64', False), requires_grad=True)
    F = step.create_boundary_force_op(core).apply(x)
    (g,) = torch.autograd.grad(F.sum(), x)
    assert torch.equal(F, torch.zeros(2, dtype=torch.float64)) and not g.any()
    out, Ft = step.create_timestep_op(2, boundary_force_outputs=core).apply(x)
    (g,) = torch.autograd.grad(Ft.sum(), x)
    assert not Ft.any() and tuple(Ft.shape) == (2, 2) and not g.any()
    full, _, _ = _make('D2Q9', shape, bodies=False)
    every = lbm.NoSlip('everything')
    full.set_boundary_including_adjoint(every)
    assert full.boundary_links(every).n == 0
    F = full.create_boundary_force_op(every).apply(x)
    (g,) = torch.autograd.grad(F.sum(), x)
    assert not F.any() and not g.any()


def test_links_are_cached_and_rebuilt_after_set_boundary():
    import torch
    shape = SHAPES['D2Q9']
    step, body, lid = _make('D2Q9', shape)
    s = _state('D2Q9', shape, 'float64', False)
    op = step.create_boundary_force_op(body)
    first = step.boundary_links(body)
    assert step.boundary_links(body) is first
    F1 = op.apply(torch.tensor(s)).numpy()
    more = np.zeros(shape, bool)
    more[7:9, 4:6] = True
    step.set_boundary_including_adjoint(body, mask_array=more)
    assert step.boundary_links(body) is not first and step.boundary_links(body).n > first.n
    assert step._force_tables.keys() <= {body}              # (the tables' memo is dropped with the lists)
    F2 = op.apply(torch.tensor(s)).numpy()
    flags = step.boundary_handling.flags
    F, A, n, _ = _reference('D2Q9', flags, step.boundary_handling.conditions[body], s, False)
    assert n == step.boundary_links(body).n and (np.abs(F2 - F) <= _bound(F, A, n, 'float64')).all()
    assert np.abs(F2 - F1).max() > 1e-3


# --- the sources -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx,addr', [('int', 'buf'), ('int', 'ptr'), ('long long', 'ptr')])
@pytest.mark.parametrize('dtype', ['float32', 'float16', 'float64'])
def test_boundary_force_sources_compile(idx, addr, dtype):
    """The three addressing variants compile to gfx950 code objects without a device, and carry the three kernels."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    from tests.test_native_abi import _is_amdgpu_elf
    K = lbm.WallForceKernels(lbm.LBStencil('D3Q19'), dtype, 'gpu')
    src = K.source(idx, addr)
    assert f'typedef {idx} IDX;' in src and ('make_buffer_rsrc' in src) == (addr == 'buf')
    assert 'atomic' not in src.lower()
    code = rt.compile_hip(src, name='psad_lbm_wall_force.hip')
    assert _is_amdgpu_elf(code)
    for nm in ('lbm_wall_force', 'lbm_wall_force_sum', 'lbm_wall_force_adj'):
        assert nm.encode() in code
    assert len(K.build()) == 3


def test_block_count_is_a_function_of_the_link_count():
    from pystencils_autodiff_amd.lbm._wall_force import DEFAULT_BLOCK_CAP, WallForceKernels
    assert [WallForceKernels.blocks(n) for n in (1, 256, 257, 256 * DEFAULT_BLOCK_CAP + 1)] == \
        [1, 1, 2, DEFAULT_BLOCK_CAP]
    assert [WallForceKernels.blocks(700, cap) for cap in (1, 2, 3, 4)] == [1, 2, 3, 3]


# --- GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('stencil,kind,dtype,zc', FORCE_CASES)
def test_force_gpu_vs_reference(stencil, kind, dtype, zc):
    """The HIP kernels, the CPU cases and bounds (float16: the reference runs on the same half-rounded state, so only
    the kernel's arithmetic is measured)."""
    _force_case(stencil, kind, dtype, zc, 'gpu')


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,kind,dtype', [('D2Q9', 'noslip', 'float64'), ('D2Q9', 'ubb', 'float32'),
                                                ('D2Q9', 'noslip', 'float16'), ('D3Q19', 'ubb', 'float64'),
                                                ('D3Q19', 'noslip', 'float32'), ('D3Q27', 'noslip', 'float64'),
                                                ('D3Q27', 'ubb', 'float32')])
def test_backward_gpu_is_the_coefficient_array(stencil, kind, dtype):
    g = _backward_case(stencil, kind, dtype, False, 'gpu')
    assert np.array_equal(g, _backward_case(stencil, kind, dtype, False, 'gpu'))


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,kind,dtype,zc', [('D2Q9', 'ubb', 'float32', True), ('D3Q19', 'noslip', 'float64', False),
                                                   ('D3Q19', 'ubb', 'float16', False)])
def test_force_gpu_against_cpu(stencil, kind, dtype, zc):
    a, ba = _force_case(stencil, kind, dtype, zc, 'gpu', 'HIP ')
    b, bb = _force_case(stencil, kind, dtype, zc, 'cpu', 'C ')
    assert (np.abs(a - b) <= ba + bb).all()


def _checkerboard(shape=(24, 20)):
    i, j = np.indices(shape)
    return shape, (i % 2 == 1) & (j % 3 == 1)                # 84 one-cell obstacles, 8 links each: 672 = 2·256 + 160


@pytest.mark.gpu
def test_reduction_shapes_gpu():
    """D2Q9 24×20 with scattered one-cell obstacles: several hundred links, no multiple of 64. The block cap forced
    to 1 (one workgroup strides over all links), to 2 (two partials, the strided loop) and the default (one workgroup
    per 256 links): each within the bound of the reference, and bitwise reproducible."""
    import torch
    shape, mask = _checkerboard()
    step, _, _ = _make('D2Q9', shape, 'float32', target='gpu', bodies=False)
    body = lbm.NoSlip('dots')
    step.set_boundary_including_adjoint(body, mask_array=mask)
    n = step.boundary_links(body).n
    assert n == 672 and n % 64 != 0 and step._wall_force_kernels().blocks(n) == 3
    s = _state('D2Q9', shape, 'float32', False)
    F, A, nr, _ = _reference('D2Q9', step.boundary_handling.flags, 1, s, False)
    assert nr == n
    bound = _bound(F, A, n, 'float32')
    for cap in (1, 2, None):
        got = _apply(step, body, s, cap=cap)
        again = _apply(step, body, s, cap=cap)
        print(f'cap {cap}: {n} links, error {np.abs(got - F)}, bound {bound}')
        assert (np.abs(got - F) <= bound).all() and np.array_equal(got, again)
    # 48×40: 2496 links, 10 partials — the second stage's eight-at-a-time loop and its remainder
    shape, mask = _checkerboard((48, 40))
    step, _, _ = _make('D2Q9', shape, 'float32', target='gpu', bodies=False)
    step.set_boundary_including_adjoint(body, mask_array=mask)
    n = step.boundary_links(body).n
    assert n == 2496 and step._wall_force_kernels().blocks(n) == 10
    s = _state('D2Q9', shape, 'float32', False)
    F, A, nr, _ = _reference('D2Q9', step.boundary_handling.flags, 1, s, False)
    got, again = _apply(step, body, s), _apply(step, body, s)
    print(f'{n} links, 10 partials: error {np.abs(got - F)}, bound {_bound(F, A, n, "float32")}')
    assert nr == n and (np.abs(got - F) <= _bound(F, A, n, 'float32')).all() and np.array_equal(got, again)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float64', 'float16'])
def test_forced_addressing_variants_bitwise_gpu(monkeypatch, dtype):
    """``PSAD_LBM_ADDR=ptr`` (plain pointers) and ``ptr64`` (64-bit offsets too): force and gradient bitwise equal to
    the default (buffer) variant."""
    shape = SHAPES['D3Q19']
    s = _state('D3Q19', shape, dtype, False)
    dF = np.array([0.7, -1.3, 0.45])
    res = {}
    for env, want in ((None, ('int', 'buf')), ('ptr', ('int', 'ptr')), ('ptr64', ('long long', 'ptr'))):
        if env is None:
            monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
        else:
            monkeypatch.setenv('PSAD_LBM_ADDR', env)
        step, body, lid = _make('D3Q19', shape, dtype, target='gpu')
        res[env] = _apply(step, lid, s, grad=dF)
        assert {k[1:3] for k in step._wall_force_kernels()._fns} == {want}
    for env in ('ptr', 'ptr64'):
        assert np.array_equal(res[None][0], res[env][0]) and np.array_equal(res[None][1], res[env][1])


@pytest.mark.gpu
def test_layouts_bitwise_gpu():
    """fzyx (a plane per component), AoS and the time-step op's row-interleaved layout are read in place: bitwise
    equal forces."""
    import torch

    from pystencils_autodiff_amd.lbm._lattice_kernels import row_interleaved_empty
    shape = SHAPES['D3Q19']
    step, body, lid = _shared('D3Q19', 'float32', False, 'gpu')
    s = torch.tensor(_state('D3Q19', shape, 'float32', False), device='cuda')
    fzyx = s.permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
    rows = row_interleaved_empty(shape, 19, torch.float32, s.device)
    rows.copy_(s)
    op = step.create_boundary_force_op(body)
    got = [op.apply(t).cpu() for t in (s.contiguous(), fzyx, rows)]
    assert len({tuple(t.stride()) for t in (s, fzyx, rows)}) == 3
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]) and float(got[0].abs().max()) > 0


def _torch_force(f, fluid, wall, stencil, u=None):
    """The force as a user of the time-step op alone has to write it: rolled masks over whole states (torch)."""
    import torch
    dirs, w = OL.SETS[stencil]
    F = [0.0] * len(dirs[0])
    for d, c in enumerate(dirs):
        if not any(c):
            continue
        link = fluid & torch.roll(wall, tuple(-v for v in c), tuple(range(len(c))))
        beta = 0.0 if u is None else -6.0 * float(w[d]) * sum(ci * ui for ci, ui in zip(c, u))
        tot = (link * (2 * f[..., d] + beta)).sum()
        for a, ca in enumerate(c):
            if ca:
                F[a] = F[a] + ca * tot
    return torch.stack(F)


@pytest.mark.gpu
@pytest.mark.parametrize('stencil,shape', [('D2Q9', (37, 70)), ('D3Q19', (12, 11, 36))])
def test_timestep_op_float32_gpu(stencil, shape):
    """float32, T = 5, the UBB lid and the NoSlip body; the forces of both every step. The error of the forces, the
    pdfs and the gradient against the float64 torch reference (``oracle.lbm.run_moving_walls`` and ``_torch_force``) is
    at most 4× (the project's bound) the error of the same restatement run in float32 on the CPU. Measured on an MI355X:
    worst ratio 1.35 (D2Q9, the gradient; forces 0.35 – 0.49) and 1.24 (D3Q19; forces 0.39 – 0.57)."""
    import torch
    T, D = 5, len(shape)
    step, body, lid = _shared(stencil, 'float32', False, 'gpu', shape)
    mb, ml = _masks(shape)
    x = torch.tensor(_init(stencil, shape, True, seed=4), dtype=torch.float32, device='cuda', requires_grad=True)
    outs = step.create_timestep_op(T, boundary_force_outputs=[body, lid]).apply(x)
    rng = np.random.default_rng(9)
    seeds = [rng.standard_normal(tuple(o.shape)) for o in outs]
    (gx,) = torch.autograd.grad(_weighted(outs, [torch.tensor(v, dtype=torch.float32, device='cuda') for v in seeds]), x)
    got = [o.detach().double().cpu() for o in outs] + [gx.double().cpu()]
    wall, fluid = torch.tensor(mb | ml), torch.tensor(~(mb | ml))
    wv = np.zeros(shape + (D,))
    wv[ml] = UBB_U[D]
    ref = {}
    for dt in (torch.float64, torch.float32):
        f = x.detach().cpu().to(dt).requires_grad_()
        s, Fb, Fl = f, [], []
        for _ in range(T):
            s = OL.run_moving_walls(s, OMEGA, wall, torch.tensor(wv, dtype=dt), 1, stencil, True, xp=torch)
            Fb.append(_torch_force(s, fluid, torch.tensor(mb), stencil))
            Fl.append(_torch_force(s, fluid, torch.tensor(ml), stencil, UBB_U[D]))
        o = [s, torch.stack(Fb), torch.stack(Fl)]
        (g,) = torch.autograd.grad(_weighted(o, [torch.tensor(v, dtype=dt) for v in seeds]), f)
        ref[dt] = [t.detach().double() for t in o] + [g.double()]
    worst = 0.0
    for name, a, r64, r32 in zip(('pdfs', 'force body', 'force lid', 'gradient'), got, ref[torch.float64],
                                 ref[torch.float32]):
        e_gpu, e_ref = float((a - r64).abs().max()), float((r32 - r64).abs().max())
        worst = max(worst, e_gpu / e_ref)
        print(f'{stencil} {name}: error {e_gpu:.3e}, float32 restatement {e_ref:.3e}, ratio {e_gpu / e_ref:.3f} '
              '(bound 4)')
        assert e_gpu <= 4 * e_ref, name
    print(f'{stencil}: worst ratio {worst:.3f}')
