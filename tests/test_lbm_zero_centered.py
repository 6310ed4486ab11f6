"""Zero-centred pdf storage (``create_lb_update_rule(zero_centered=True)``): the pdf arrays hold ``δf_i = f_i − w_i``.

Reference: ``oracle/lbm.py`` in float64, driven from here — a zero-centred state goes in as ``δf + w`` and comes out
``− w`` (``stored_step``), obstacle cells keep what they hold; the adjoint is torch's reverse mode through that step.
The helpers (``Lattice``, ``chain``, ``chain_adjoint``) also serve ``tests/test_lbm_fp16.py``, which rounds the stored
value after every step.

CPU: three steps and their adjoint at 1e-12 on the lattice C kernels and on the rule's AutoDiffOp kernels
(``PSAD_LBM_LATTICE=0``: periodic lattices only — walls need the lattice schedule; every Guo rule but D3Q19 MRT,
whose generic derivation takes 260 s), the end-to-end op against the
plain rule's, what raises, and the emitted HIP sources (compiled for gfx950, pinned in
``tests/golden/lattice_fp16_source_sha.json``)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import sympy as sp

from oracle import lbm as OL
from pystencils_autodiff_amd import lbm
from tests import test_lbm as TL
from tests.test_native_abi import _is_amdgpu_elf

FORCE = (1e-3, -2e-3, 5e-4)
MRT_RATES = dict(bulk=1.1, third=0.9, fourth=1.2)
GOLDEN_DIR = os.path.join(os.path.dirname(__file__), 'golden')


def weights(stencil):
    return np.array([float(w) for w in OL.SETS[stencil][1]])


class Lattice:
    """One lattice of the tests: the rule's options, its walls, the step that runs it and its float64 restatement."""

    def __init__(self, stencil, shape, method='srt', compressible=True, force_model=None, walls=None, layout='fzyx',
                 omega=1.3):
        self.stencil, self.shape, self.method, self.compressible = stencil, tuple(shape), method, compressible
        self.force_model, self.walls, self.layout, self.omega = force_model, walls, layout, omega
        self.force = FORCE[:len(shape)] if force_model else None
        self.omega_odd = OL.trt_odd_rate(omega) if method == 'trt' else None
        self.mrt = OL.mrt_matrix(stencil, dict(MRT_RATES, shear=omega)) if method == 'mrt' else None
        self.wall = self.velocity = None
        if walls == 'channel':
            self.wall = TL._channel(self.shape)
        elif walls == 'cavity':
            self.wall, self.velocity = TL._cavity(self.shape)

    def rule(self, dtype, zero_centered):
        kw = {}
        if self.method == 'trt':
            kw = dict(method='trt')
        elif self.method == 'mrt':
            kw = dict(method='mrt', relaxation_rates=[sp.Symbol('omega')] + [MRT_RATES[k] for k in
                                                                             ('bulk', 'third', 'fourth')])
        if self.force_model:
            kw.update(force_model=self.force_model, force=self.force)
        if zero_centered:                       # (plain storage: the call as it was before the argument existed)
            kw['zero_centered'] = True
        return lbm.create_lb_update_rule(self.stencil, compressible=self.compressible, data_type=dtype,
                                         layout=self.layout, **kw)

    def step(self, dtype, zero_centered, target, schedule='lattice'):
        old = os.environ.get('PSAD_LBM_LATTICE')
        os.environ['PSAD_LBM_LATTICE'] = '1' if schedule == 'lattice' else '0'
        try:
            step = lbm.AutoDiffLatticeBoltzmannStep(self.rule(dtype, zero_centered), domain_size=self.shape,
                                                    relaxation_rate=self.omega, target=target)
        finally:
            if old is None:
                os.environ.pop('PSAD_LBM_LATTICE')
            else:
                os.environ['PSAD_LBM_LATTICE'] = old
        assert (step._lattice is not None) == (schedule == 'lattice')
        if self.walls == 'channel':
            TL._set_channel(step, self.shape)
        elif self.walls == 'cavity':
            TL._set_cavity(step, self.shape)
        return step

    def true_step(self, f):
        """One step of the restatement on the pdfs ``f`` (a torch tensor of any float dtype)."""
        import torch
        if self.wall is None:
            s = OL.stream(f, self.stencil, torch)
        else:
            vel = torch.tensor(self.velocity if self.velocity is not None else np.zeros(self.shape + (len(self.shape),)),
                               dtype=f.dtype)
            s = OL.stream_moving_walls(f, self.stencil, torch.tensor(self.wall), vel, torch)
        new = OL.collide(s, self.omega, self.stencil, self.compressible, torch, self.force_model, self.force,
                         self.omega_odd, self.mrt)
        return new if self.wall is None else torch.where(torch.tensor(self.wall).unsqueeze(-1), f, new)

    def stored_step(self, x, zero_centered):
        """... on the stored values ``x`` (``δf`` or ``f``): ``δf + w`` in, ``− w`` out."""
        import torch
        if not zero_centered:
            return self.true_step(x)
        w = torch.tensor(weights(self.stencil), dtype=x.dtype)
        new = self.true_step(x + w) - w
        # (an obstacle cell keeps its stored bits: a raw copy, not (x + w) − w)
        return new if self.wall is None else torch.where(torch.tensor(self.wall).unsqueeze(-1), x, new)

    def initial(self, zero_centered, seed=0):
        """Stored initial values (float64): ``tests.test_lbm._init``'s pdfs, minus the weights when zero-centred."""
        f0 = TL._init(self.stencil, self.shape, self.compressible, seed=seed)
        return f0 - weights(self.stencil) if zero_centered else f0


def _identity(a):
    return a


def chain(lat, x0, T, zero_centered, store=_identity, dtype='float64'):
    """The stored states 0 … T (numpy float64) of T steps evaluated in ``dtype``, ``store`` applied to every step's
    result (the rounding of the kernels' store)."""
    import torch
    states = [np.asarray(x0, np.float64)]
    for _ in range(T):
        x = torch.tensor(states[-1], dtype=getattr(torch, dtype))
        states.append(store(lat.stored_step(x, zero_centered).double().numpy()))
    return states


def chain_adjoint(lat, states, g, zero_centered, store=_identity, dtype='float64'):
    """The adjoint of ``chain`` from the seed ``g``: torch's reverse mode through each step at its recorded state (the
    roundings are the identity for the gradient), ``store`` applied to every step's gradient."""
    import torch
    tdt = getattr(torch, dtype)
    g = np.asarray(g, np.float64)
    for x in reversed(states[:-1]):
        xt = torch.tensor(x, dtype=tdt, requires_grad=True)
        (gx,) = torch.autograd.grad(lat.stored_step(xt, zero_centered), xt, torch.tensor(g, dtype=tdt))
        g = store(gx.double().numpy())
    return g


def run_cpu(step, x0, g, T):
    """T steps and their adjoint on the step's own arrays (the C kernels): (result, gradient) as float64."""
    step.set_pdfs(x0)
    step.run(T, record=True)
    out = np.array(step.pdf_array, dtype=np.float64)
    step.set_adjoint_pdfs(g)
    step.run_backward(T)
    return out, np.array(step.adjoint_pdf_array, dtype=np.float64)


# (id, lattice, schedules): a Guo force on a periodic lattice, a no-slip channel with its obstacle (walls need the
# lattice schedule), and a periodic lattice without a force. On the AutoDiffOp schedule the last one takes the adjoint
# of ``create_lb_adjoint_rule`` and a Guo rule the generic transposed derivation, whose sympy time grows with Q and
# with the MRT matrix: building the step and one forward and one adjoint step takes 12 s for D2Q9 MRT, 22 s for D3Q19
# SRT, 42 s for D3Q19 TRT — and 260 s for D3Q19 MRT, the one Guo case that schedule leaves out
CPU_LATTICES = [(f'{st}-{m}-{kind}', Lattice(st, shape, m, comp, **kw),
                 sched if (kind, st, m) != ('guo', 'D3Q19', 'mrt') else ('lattice',))
                for st, shape in (('D2Q9', (9, 7)), ('D3Q19', (5, 6, 4)))
                for m, comp in (('srt', True), ('trt', False), ('mrt', True))
                for kind, kw, sched in (('guo', dict(force_model='guo'), ('lattice', 'autodiffop')),
                                        ('channel', dict(walls='channel', layout='numpy'), ('lattice',)),
                                        ('periodic', dict(), ('autodiffop',)))]
CPU_CASES = [(name, sched) for name, _, scheds in CPU_LATTICES for sched in scheds]


@pytest.mark.parametrize('name,schedule', CPU_CASES)
def test_zero_centered_cpu_vs_oracle(name, schedule):
    """float64, T = 3: the zero-centred states and the adjoint of the three steps at 1e-12 of the largest reference
    value, against the oracle fed ``δf + w`` (and, as a control of that reference, the plain rule against it too)."""
    lat = next(c[1] for c in CPU_LATTICES if c[0] == name)
    T = 3
    g = np.random.default_rng(11).standard_normal(lat.shape + (len(weights(lat.stencil)),))
    # (the plain rule's run controls the reference; a Guo rule's AutoDiffOp derivation is slow, and that control has
    # run on the lattice schedule of the same lattice)
    for zc in (True, False) if schedule == 'lattice' or lat.force_model is None else (True,):
        x0 = lat.initial(zc, seed=3)
        states = chain(lat, x0, T, zc)
        gref = chain_adjoint(lat, states, g, zc)
        step = lat.step('float64', zc, 'cpu', schedule)
        assert getattr(step._update_rule, 'zero_centered') is zc
        out, grad = run_cpu(step, x0, g, T)
        ef, eg = np.abs(out - states[-1]).max(), np.abs(grad - gref).max()
        print(f'{name} {schedule} zero_centered={zc}: forward {ef:.2e} of {np.abs(states[-1]).max():.2e}, '
              f'adjoint {eg:.2e} of {np.abs(gref).max():.2e}')
        assert ef <= 1e-12 * np.abs(states[-1]).max()
        assert eg <= 1e-12 * np.abs(gref).max()
    # the two storages describe one flow
    plain = chain(lat, lat.initial(False, seed=3), T, False)[-1]
    assert np.abs(plain - weights(lat.stencil) - chain(lat, lat.initial(True, seed=3), T, True)[-1]).max() <= 1e-14


def test_zero_centered_rule_and_macroscopic_ops():
    """The rule's flag, the getter's ``ρ = 1 + Σ δf`` with the momentum unchanged, the setter's ``feq − w``."""
    import torch
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, zero_centered=True)
    assert rule.zero_centered is True
    assert lbm.create_lb_update_rule('D2Q9').zero_centered is False
    assert lbm.macroscopic_setter is lbm.equilibrium_setter
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(6, 5), relaxation_rate=1.0, target='cpu')
    assert step._lattice is not None and step._lattice_kernels().zero_centered
    setter, getter = step.create_macroscopic_setter_op(), step.create_macroscopic_getter_op()
    rng = np.random.default_rng(2)
    rho = torch.tensor(1 + 0.1 * rng.standard_normal((6, 5)))
    vel = torch.tensor(0.05 * rng.standard_normal((6, 5, 2)))
    (pdfs,) = setter.apply(rho, vel)
    assert np.abs(pdfs.numpy() + weights('D2Q9') - OL.equilibrium(rho.numpy(), vel.numpy(), 'D2Q9', True)).max() < 1e-14
    r2, v2 = getter.apply(pdfs)
    assert np.abs(r2.numpy() - rho.numpy()).max() < 1e-13 and np.abs(v2.numpy() - vel.numpy()).max() < 1e-13


def test_zero_centered_end_to_end_equals_plain_rule():
    """``create_end_to_end_op`` (ρ, u → equilibrium → T steps in a no-slip channel → ρ, u) on a zero-centred step
    equals the same op on the plain rule in ρ, u and the gradients of a scalar loss, at 1e-12 of each one's maximum;
    the pdfs between are the plain ones minus the weights."""
    import torch
    shape, T = (10, 8), 4
    rng = np.random.default_rng(12)
    rho0, u0 = 1 + 0.05 * rng.standard_normal(shape), 0.03 * rng.standard_normal(shape + (2,))
    wt = torch.tensor(rng.standard_normal(shape + (2,)))
    res = {}
    for zc in (False, True):
        rule = lbm.create_lb_update_rule('D2Q9', compressible=True, zero_centered=zc)
        step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.4, target='cpu')
        TL._set_channel(step, shape, obstacle=False)
        rho, vel = torch.tensor(rho0, requires_grad=True), torch.tensor(u0, requires_grad=True)
        r = step.create_end_to_end_op(T, vel, rho, num_times_steps_without_save=1)
        ((r.output_velocity_tensor * wt).sum() + (r.output_density_tensor ** 2).sum()).backward()
        res[zc] = dict(rho=r.output_density_tensor.detach(), vel=r.output_velocity_tensor.detach(), drho=rho.grad,
                       dvel=vel.grad, pdf_in=r.input_pdf_tensor.detach(), pdf_out=r.output_pdf_tensor.detach())
    for k in ('rho', 'vel', 'drho', 'dvel'):
        a, b = res[False][k], res[True][k]
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), k
    w = torch.tensor(weights('D2Q9'))
    for k in ('pdf_in', 'pdf_out'):
        assert float((res[False][k] - w - res[True][k]).abs().max()) <= 1e-14, k


def test_zero_centered_field_rules_stay_on_the_lattice_kernels():
    """Per-cell ω with zero-centred float64 pdfs needs no extra code: one step and ``dω`` against the oracle."""
    import torch
    from pystencils_autodiff_amd import ps
    shape = (8, 6)
    wf = ps.fields('omega_f: float64[2D]')
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, relaxation_rate=wf.center, zero_centered=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, target='cpu')
    assert step._lattice is not None and step._lattice_kernels().omega_field
    rng = np.random.default_rng(5)
    x0 = TL._init('D2Q9', shape, True, seed=6) - weights('D2Q9')
    om = 1.3 + 0.2 * rng.standard_normal(shape)
    g = rng.standard_normal(x0.shape)
    xt, wt = torch.tensor(x0, requires_grad=True), torch.tensor(om, requires_grad=True)
    w = torch.tensor(weights('D2Q9'))
    ref = OL.step(xt + w, wt, 'D2Q9', True, xp=torch) - w
    gx, gw = torch.autograd.grad(ref, (xt, wt), torch.tensor(g))
    x = torch.tensor(x0, requires_grad=True)
    wv = torch.tensor(om, requires_grad=True)
    out = step.create_timestep_op(1).apply(x, wv)
    out.backward(torch.tensor(g))
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-13
    assert float((x.grad - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert float((wv.grad - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


@pytest.mark.parametrize('model', ['simple', 'guo'])
def test_zero_centered_force_field_stays_on_the_lattice_kernels(model):
    """A per-cell force with zero-centred float64 pdfs likewise: three steps, the pdf adjoint and ``dF`` summed over the
    steps against the oracle."""
    import torch
    from pystencils_autodiff_amd import ps
    shape, T = (8, 6), 3
    F = ps.fields('F(2): float64[2D]')
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, force_model=model, force=F, zero_centered=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.4, target='cpu')
    assert step._lattice is not None and step._lattice_kernels().force_field and step._lattice_kernels().zero_centered
    rng = np.random.default_rng(7)
    x0 = TL._init('D2Q9', shape, True, seed=8) - weights('D2Q9')
    Fv = 1e-3 * rng.standard_normal(shape + (2,))
    g = rng.standard_normal(x0.shape)
    w = torch.tensor(weights('D2Q9'))
    xt, Ft = torch.tensor(x0, requires_grad=True), torch.tensor(Fv, requires_grad=True)
    ref = OL.run(xt + w, 1.4, T, 'D2Q9', True, xp=torch, force_model=model, force=(Ft[..., 0], Ft[..., 1])) - w
    gx, gF = torch.autograd.grad(ref, (xt, Ft), torch.tensor(g))
    x, Fx = torch.tensor(x0, requires_grad=True), torch.tensor(Fv, requires_grad=True)
    out = step.create_timestep_op(T).apply(x, Fx)
    out.backward(torch.tensor(g))
    assert float((out.detach() - ref.detach()).abs().max()) <= 1e-12 * float(ref.detach().abs().max())
    assert float((x.grad - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    assert float((Fx.grad - gF).abs().max()) <= 1e-12 * float(gF.abs().max())


# --- what raises ------------------------------------------------------------------------------------------------------
def density_boundaries(D=2):
    """Boundaries whose links read a density: a link program, a neighbour link, a density-weighted moving wall."""
    return [lbm.FixedDensity(1.02), lbm.FreeSlip((0, 1) + (0,) * (D - 2)),
            lbm.UBB((0.05,) + (0.0,) * (D - 1), density_weighted=True)]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_zero_centered_density_links_raise(which):
    """``FixedDensity``, ``FreeSlip`` and a density-weighted ``UBB`` on a zero-centred step raise a
    ``NotImplementedError`` that names ``zero_centered`` (at the step, and in the kernels' description itself); the
    plain ``UBB`` and ``NoSlip`` are taken."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    bc = density_boundaries()[which]
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, zero_centered=True)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(8, 6), relaxation_rate=1.3, target='cpu')
    with pytest.raises(NotImplementedError, match='zero_centered'):
        step.set_boundary_including_adjoint(bc, lbm.make_slice[:, 0])
    assert not step.boundary_handling.has_walls
    step.set_boundary_including_adjoint(lbm.UBB((0.05, 0.0)), lbm.make_slice[:, 0])
    step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, -1])
    assert step._lattice_kernels().links is not None
    # the kernels: the same lattice description with the plain rule's tables
    plain = lbm.AutoDiffLatticeBoltzmannStep(lbm.create_lb_update_rule('D2Q9', compressible=True), domain_size=(8, 6),
                                             relaxation_rate=1.3, target='cpu')
    plain.set_boundary_including_adjoint(bc, lbm.make_slice[:, 0])
    K = plain._lattice_kernels()
    with pytest.raises(NotImplementedError, match='zero_centered'):
        LatticeKernels(K.stencil, True, np.float64, True, 'cpu', K.links, programs=K.programs, zero_centered=True)


# --- emitted sources --------------------------------------------------------------------------------------------------
def _golden_module():
    spec = importlib.util.spec_from_file_location('make_lattice_fp16_golden',
                                                  os.path.join(GOLDEN_DIR, 'make_lattice_fp16_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_variant_sources_pinned():
    """Every emitted source of the float16 / zero-centred variants (``make_lattice_fp16_golden.VARIANTS``: C, and HIP
    for both index types and addressing modes) is the pinned one; the default of both flags prints the sources the
    emitter printed before they existed (``test_lbm_neighbour_links`` has those pins)."""
    mod = _golden_module()
    with open(mod.PATH) as fh:
        golden = json.load(fh)
    shas = mod.shas()
    assert sorted(shas) == sorted(golden)
    assert [k for k in golden if shas[k] != golden[k]] == []
    K = mod.kernels('D2Q9-srt-noslip', 'float32', False, 'gpu')
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    old = LatticeKernels(K.stencil, K.compressible, np.float32, K.walls, 'gpu', K.links, K.force_model, K.force)
    assert hashlib.sha256(K.source().encode()).hexdigest() == hashlib.sha256(old.source().encode()).hexdigest()


def test_new_variant_sources_compile_for_gfx950():
    """The HIP sources of the float16 and the zero-centred variants compile to gfx950 code objects with their entry
    points: 2-byte buffer accesses in ``buf`` mode, plain ``_Float16`` indexing in ``ptr`` mode, the shift in both."""
    from pystencils_autodiff_amd.backends import hip_runtime as rt
    mod = _golden_module()
    for name, dtype, zc in (('D2Q9-srt-cavity', 'float16', True), ('D3Q19-trt-channel-guo', 'float16', False),
                            ('D2Q9-mrt-periodic-simple', 'float16', True), ('D3Q19-srt-channel', 'float32', True),
                            ('D2Q9-srt-cavity', 'float64', True)):
        K = mod.kernels(name, dtype, zc, 'gpu')
        for idx, addr in (('int', 'buf'), ('int', 'ptr'), ('long long', 'ptr')):
            src = K.source(idx, addr)
            assert ('typedef _Float16 T;' in src) == (dtype == 'float16')
            assert ('raw_buffer_load_b16' in src) == (dtype == 'float16' and addr == 'buf')
            assert ('raw_buffer_store_b16' in src) == (dtype == 'float16' and addr == 'buf')
            w0 = repr(float(K.stencil.weights[0]))
            assert (f' + ({K.ct}){w0};' in src) == zc and (f' - ({K.ct}){w0})' in src) == zc
            code = rt.compile_hip(src, name='psad_lbm.hip')
            assert _is_amdgpu_elf(code) and b'lbm_fwd' in code and b'lbm_adj' in code
        assert len(K.build()) == 3
