"""float16 pdf storage on the lattice kernels (float32 arithmetic, stores rounded to nearest-even), plain and
zero-centred.

Reference: ``oracle/lbm.py`` in float64 on the float16 inputs cast to float64 (``test_lbm_zero_centered.Lattice``); over
T steps the stored value is rounded to float16 after every step, as the kernels' stores do, and the adjoint is torch's
reverse mode through each step at its recorded state with the gradient rounded where the kernels store it.

Bounds. One step, per element: ``|out − ref| ≤ ½ ulp16(ref) + 1e-5 max|ref|`` — the rounding of the store plus the
tolerance the float32 lattice tests of ``tests/test_lbm.py`` give the float32 arithmetic before it; ``ulp16`` is the
float16 grid spacing of the binade that holds ``|ref|`` (a binade's end is a grid point of both neighbours, so a
correctly rounded store never needs the wider one). T = 3: the error against the float64 chain is at most 4× the error
of the same chain evaluated in float32 on the CPU (the convention of ``tests/test_lbm_omega_field.py``); both errors
are whole float16 steps at the elements where a store rounded the other way, and ``three_step_reference`` chooses
inputs at which the float32 chain has such an element among the large values — so this bound is never tighter than
one float16 step of the largest value, anywhere."""
import numpy as np
import pytest

from pystencils_autodiff_amd import lbm, ps
from tests.test_lbm_zero_centered import Lattice, chain, chain_adjoint, density_boundaries, run_cpu, weights


def r16(a):
    """Round to float16 (nearest-even), as float64."""
    return np.asarray(a).astype(np.float16).astype(np.float64)


def ulp16(a):
    """The float16 grid spacing at ``|a|``: 2^(e − 10) in the binade 2^e ≤ |a| < 2^(e + 1), 2^-24 below 2^-14."""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def worst(out, ref):
    """max over the elements of |out − ref| / (½ ulp16(ref) + 1e-5 max|ref|): the one-step bound holds iff ≤ 1."""
    return float((np.abs(out - ref) / (0.5 * ulp16(ref) + 1e-5 * np.abs(ref).max())).max())


# name → lattice. Together: D2Q9 / D3Q19 / D3Q27, SRT / TRT (magic number) / MRT, compressible and not, fzyx and AoS
# pdfs, periodic / a no-slip channel with its obstacle / a lid-driven cavity (UBB: affine links with constant
# coefficients), constant 'simple' and 'guo' forces
CPU_LATTICES = {
    'D2Q9-srt-periodic': Lattice('D2Q9', (9, 7)),
    'D2Q9-wrap': Lattice('D2Q9', (2, 2), compressible=False, layout='numpy'),
    'D2Q9-trt-channel-aos': Lattice('D2Q9', (10, 8), 'trt', False, walls='channel', layout='numpy'),
    'D2Q9-srt-cavity': Lattice('D2Q9', (9, 8), walls='cavity'),
    'D2Q9-mrt-guo': Lattice('D2Q9', (9, 7), 'mrt', True, 'guo'),
    'D2Q9-mrt-simple': Lattice('D2Q9', (9, 7), 'mrt', False, 'simple'),
    'D2Q9-trt-cavity-simple': Lattice('D2Q9', (8, 9), 'trt', True, 'simple', walls='cavity', layout='numpy'),
    'D3Q19-srt-channel-guo': Lattice('D3Q19', (7, 8, 6), 'srt', False, 'guo', walls='channel'),
    'D3Q19-trt-periodic-aos': Lattice('D3Q19', (5, 6, 4), 'trt', True, layout='numpy'),
    'D3Q19-mrt-channel': Lattice('D3Q19', (7, 8, 6), 'mrt', True, walls='channel'),
    'D3Q27-srt-channel': Lattice('D3Q27', (7, 8, 6), walls='channel'),
}
_REFS = {}


def one_step_reference(lattices, name, zc, seed=21):
    """(stored float16 input, seed, float64 result of one step, float64 adjoint of it) — computed once per case."""
    key = (id(lattices), name, zc, seed)
    if key not in _REFS:
        lat = lattices[name]
        x0 = r16(lat.initial(zc, seed=seed))
        g = r16(np.random.default_rng(seed + 1).standard_normal(x0.shape))
        states = chain(lat, x0, 1, zc)
        _REFS[key] = x0, g, states[1], chain_adjoint(lat, states, g, zc)
    return _REFS[key]


@pytest.mark.parametrize('zc', [False, True], ids=['plain', 'zero-centred'])
@pytest.mark.parametrize('name', list(CPU_LATTICES))
def test_fp16_lattice_cpu_one_step(name, zc):
    """float16 pdfs run on the lattice C kernels (``uint16_t`` bits, float32 arithmetic): one step and one adjoint
    step inside the one-step bound, obstacle cells bit for bit what they held."""
    lat = CPU_LATTICES[name]
    step = lat.step('float16', zc, 'cpu')
    assert step._lattice is not None
    K = step._lattice_kernels()
    assert K.dtype == np.float16 and K.ct == 'float' and K.zero_centered is zc and 'psad_f2h' in K.source()
    x0, g, ref, gref = one_step_reference(CPU_LATTICES, name, zc)
    out, grad = run_cpu(step, x0.astype(np.float16), g.astype(np.float16), 1)
    assert step.pdf_array.dtype == np.float16 and step.adjoint_pdf_array.dtype == np.float16
    wf, wg = worst(out, ref), worst(grad, gref)
    print(f'{name} zero_centered={zc}: forward {wf:.3f}, adjoint {wg:.3f} of the bound; max|ref| '
          f'{np.abs(ref).max():.3e}')
    assert wf <= 1.0 and wg <= 1.0
    if lat.wall is not None:
        assert np.array_equal(out[lat.wall], x0[lat.wall]) and np.array_equal(grad[lat.wall], g[lat.wall])


def test_fp16_obstacle_cells_keep_their_bits():
    """An obstacle cell's copy (``dst = src``, ``out = g``) moves the stored 16 bits, unconverted: quiet and
    signalling NaN payloads, infinities and subnormals come out as they went in."""
    lat = CPU_LATTICES['D2Q9-trt-channel-aos']
    x0, g, _, _ = one_step_reference(CPU_LATTICES, 'D2Q9-trt-channel-aos', True)
    x, gg = x0.astype(np.float16), g.astype(np.float16)
    odd = np.array([0x7e01, 0x7d01, 0xfc00, 0x0001, 0x8000, 0xfdff, 0x7c00, 0x03ff, 0xffff], np.uint16)
    cell = tuple(np.argwhere(lat.wall)[3])
    x.view(np.uint16)[cell] = odd
    gg.view(np.uint16)[cell] = odd[::-1]
    step = lat.step('float16', True, 'cpu')
    step.set_pdfs(x)
    step.run(1, record=True)
    assert np.array_equal(np.asarray(step.pdf_array).view(np.uint16)[cell], odd)
    step.set_adjoint_pdfs(gg)
    step.run_backward(1)
    assert np.array_equal(np.asarray(step.adjoint_pdf_array).view(np.uint16)[cell], odd[::-1])


def three_step_reference(lat, zc, T=3):
    """Stored input and seed, then (result, gradient) of the float64 chain and of the same chain in float32, both
    rounding to float16 after every step — once per case.
    The two chains differ only where a store rounded the other way, by whole float16 steps; on a small lattice the
    float32 chain may have no such element at all, or only among the small values. The inputs are therefore the first
    seed (31, 32, …) at which the float32 chain's own error reaches a quarter of a float16 step of the largest
    reference value, in the result and in the gradient — 4× of it then covers one step anywhere: a property of the two
    reference chains alone."""
    key = ('T3', id(lat), zc)
    if key in _REFS:
        return _REFS[key]
    def far(a32, a64):
        return np.abs(a32 - a64).max() >= 0.25 * ulp16(np.abs(a64).max())
    # (the (2, 2) lattice has 36 values: a store of its float32 chain rounds the other way at one seed in hundreds)
    for seed in range(31, 159 if int(np.prod(lat.shape)) >= 64 else 1031):
        x0 = r16(lat.initial(zc, seed=seed))
        states = {dtype: chain(lat, x0, T, zc, r16, dtype) for dtype in ('float64', 'float32')}
        if not far(states['float32'][-1], states['float64'][-1]):
            continue
        g = r16(np.random.default_rng(seed + 1000).standard_normal(x0.shape))
        grads = {dtype: chain_adjoint(lat, st, g, zc, r16, dtype) for dtype, st in states.items()}
        if far(grads['float32'], grads['float64']):
            _REFS[key] = x0, g, (states['float64'][-1], grads['float64']), (states['float32'][-1], grads['float32'])
            return _REFS[key]
    pytest.fail('no seed at which the float32 chain differs from the float64 chain in the large values')


def check_three_steps(tag, out, grad, ref64, ref32):
    for what, got, r64, r32 in (('forward', out, ref64[0], ref32[0]), ('adjoint', grad, ref64[1], ref32[1])):
        e, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
        print(f'{tag} {what}: error {e:.3e}, float32 chain {e32:.3e}, ratio {e / e32:.3f} (bound 4); ulp16 at '
              f'max|ref| {float(ulp16(np.abs(r64).max())):.3e}')
        assert e <= 4 * e32, (tag, what)


def test_fp16_timestep_op_cpu():
    """``create_timestep_op`` on the C kernels takes and returns float16 tensors (the gradient's dtype is the
    input's) and gives, bit for bit, what ``run`` / ``run_backward`` give on the step's own arrays."""
    import torch
    lat = CPU_LATTICES['D2Q9-trt-channel-aos']
    x0, g, _, _ = one_step_reference(CPU_LATTICES, 'D2Q9-trt-channel-aos', True)
    step = lat.step('float16', True, 'cpu')
    x = torch.tensor(x0, dtype=torch.float16, requires_grad=True)
    out = step.create_timestep_op(3).apply(x)
    out.backward(torch.tensor(g, dtype=torch.float16))
    assert out.dtype == torch.float16 and x.grad.dtype == torch.float16
    ref, gref = run_cpu(lat.step('float16', True, 'cpu'), x0.astype(np.float16), g.astype(np.float16), 3)
    assert np.array_equal(out.detach().double().numpy(), ref) and np.array_equal(x.grad.double().numpy(), gref)


def _fallback_inputs(lat, name):
    """The first seed (21, 22, …) at which no element of the float64 result or gradient of one step lies below 2^-11:
    there a float16 step is at least 2^-21 = 4.8e-7, above the absolute error of float32 arithmetic on values of
    order one (a few 2^-24) — below it two correct float32 evaluations may round more than one float16 step apart."""
    for seed in range(21, 85):
        x0, g, ref, gref = one_step_reference(CPU_LATTICES, name, False, seed)
        if min(np.abs(ref).min(), np.abs(gref).min()) >= 2.0 ** -11:
            return x0, g, ref, gref
    pytest.fail('no seed without a near-zero reference value')


@pytest.mark.parametrize('name', ['D2Q9-srt-periodic', 'D2Q9-mrt-simple', 'D3Q19-trt-periodic-aos'])
def test_fp16_lattice_matches_autodiffop_fallback(name):
    """The lattice C kernels against the rule's AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``, what float16 rules ran on
    before; periodic: it has no walls), one step and one adjoint step: both round a float32 result of the same
    equations, so they differ in at most 1 % of the elements, by one float16 step each (``_fallback_inputs``).
    Plain storage: a zero-centred result is a cancelling difference with values down to zero among its thousands
    of elements at every seed, where one float16 step (6e-8) is below the float32 arithmetic's absolute error on the
    pdfs (1e-7) — there the two kernels are held to the one-step bound against the float64 oracle instead
    (``test_fp16_zero_centered_fallback_within_the_one_step_bound``)."""
    lat = CPU_LATTICES[name]
    x0, g, ref, gref = _fallback_inputs(lat, name)
    res = {s: run_cpu(lat.step('float16', False, 'cpu', s), x0.astype(np.float16), g.astype(np.float16), 1)
           for s in ('lattice', 'autodiffop')}
    for k, what in enumerate(('forward', 'adjoint')):
        a, b = res['lattice'][k], res['autodiffop'][k]
        differ = a != b
        print(f'{name} {what}: {int(differ.sum())} of {a.size} elements differ')
        assert np.all(np.abs(a - b)[differ] <= ulp16(np.maximum(np.abs(a), np.abs(b)))[differ])
        assert differ.mean() <= 0.01
        # (the oracle-rounded reference is inside that too: the share is not the inputs' doing)
        r = r16((ref, gref)[k])
        for c in (a, b):
            assert np.all(np.abs(c - r) <= ulp16(np.maximum(np.abs(c), np.abs(r)))) and (c != r).mean() <= 0.01


@pytest.mark.parametrize('name', ['D2Q9-srt-periodic', 'D3Q19-trt-periodic-aos'])
def test_fp16_zero_centered_fallback_within_the_one_step_bound(name):
    """Zero-centred float16 pdfs on the AutoDiffOp kernels (``PSAD_LBM_LATTICE=0``): the rule itself carries the
    shift, and one step and its adjoint are inside the one-step bound, as the lattice kernels are."""
    lat = CPU_LATTICES[name]
    x0, g, ref, gref = one_step_reference(CPU_LATTICES, name, True)
    out, grad = run_cpu(lat.step('float16', True, 'cpu', 'autodiffop'), x0.astype(np.float16), g.astype(np.float16), 1)
    assert worst(out, ref) <= 1.0 and worst(grad, gref) <= 1.0


def test_fp16_zero_centered_storage_is_more_accurate():
    """D2Q9 32×24, ω = 1.7, 50 steps on the lattice C kernels against the unrounded float64 oracle: the zero-centred
    float16 run's largest error is at most ¼ of the plain float16 run's (the oracle with a float16 rounding after
    every step gives 1.0e-5 against 3.2e-4, a ratio of 31, at a signal max|f − w| of 1.7e-2)."""
    lat = Lattice('D2Q9', (32, 24), compressible=False, omega=1.7)
    f0 = lat.initial(False)
    exact = chain(lat, f0, 50, False)[-1]
    err = {}
    for zc in (False, True):
        step = lat.step('float16', zc, 'cpu')
        assert step._lattice is not None
        w = weights('D2Q9') if zc else 0
        step.set_pdfs((f0 - w).astype(np.float16))
        step.run(50)
        err[zc] = np.abs(np.array(step.pdf_array, np.float64) + w - exact).max()
    print(f'plain {err[False]:.3e}, zero-centred {err[True]:.3e}, ratio {err[False] / err[True]:.1f}; signal '
          f'{np.abs(exact - weights("D2Q9")).max():.3e}')
    assert err[True] <= 0.25 * err[False]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_fp16_density_links_raise(which):
    """``FixedDensity``, ``FreeSlip`` and a density-weighted ``UBB`` with float16 pdfs raise a ``NotImplementedError``
    that names the dtype (their adjoint adds atomically in the storage type); ``NoSlip`` and the plain ``UBB`` are
    taken."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    bc = density_boundaries()[which]
    rule = lbm.create_lb_update_rule('D2Q9', compressible=True, data_type='float16')
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(8, 6), relaxation_rate=1.3, target='cpu')
    assert step._lattice is not None
    with pytest.raises(NotImplementedError, match='float16'):
        step.set_boundary_including_adjoint(bc, lbm.make_slice[:, 0])
    step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, 0])
    step.set_boundary_including_adjoint(lbm.UBB((0.05, 0.0)), lbm.make_slice[:, -1])
    plain = lbm.AutoDiffLatticeBoltzmannStep(lbm.create_lb_update_rule('D2Q9', compressible=True), domain_size=(8, 6),
                                             relaxation_rate=1.3, target='cpu')
    plain.set_boundary_including_adjoint(bc, lbm.make_slice[:, 0])
    K = plain._lattice_kernels()
    for target in ('cpu', 'gpu'):
        with pytest.raises(NotImplementedError, match='float16'):
            LatticeKernels(K.stencil, True, np.float16, True, target, K.links, programs=K.programs)


def test_fp16_field_rules_stay_on_the_autodiffop_kernels():
    """A per-cell ω or force with float16 pdfs still builds a step without the lattice schedule (the kernels would
    accumulate the field's adjoint over the steps in float16), and the kernels say so themselves."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    wf = ps.fields('omega_f: float16[2D]')
    F = ps.fields('F(2): float16[2D]')
    for kw in (dict(relaxation_rate=wf.center), dict(force_model='guo', force=F, relaxation_rate=1.3)):
        for zc in (False, True):
            rule = lbm.create_lb_update_rule('D2Q9', data_type='float16', zero_centered=zc, **kw)
            step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=(8, 6), target='cpu')
            assert step._lattice is None
    st = lbm.LBStencil('D2Q9')
    with pytest.raises(NotImplementedError, match='float16'):
        LatticeKernels(st, True, np.float16, False, 'cpu', omega_field=True)
    with pytest.raises(NotImplementedError, match='float16'):
        LatticeKernels(st, True, np.float16, False, 'cpu', force_model='guo', force_field=True)
    with pytest.raises(NotImplementedError):
        LatticeKernels(st, True, np.int16, False, 'cpu')


def test_fp16_argument_format_and_mode():
    """ω stays a ``float`` argument; the addressing mode switches at 2³¹ bytes of 2-byte elements."""
    from pystencils_autodiff_amd.lbm._lattice_kernels import LatticeKernels
    from tests.test_lbm_addressing import I31, _meta
    K = LatticeKernels(lbm.LBStencil('D2Q9'), True, np.float16, False, 'gpu')
    fmt, om_i = K.arg_format('fwd', 'int'), [a.kind for a in K.table('fwd')].index('rate')
    assert fmt[om_i] == 'f' and fmt == 'QQQQ' + 'iii' + 'i' * 8 + 'qq' + 'f'
    assert K._mode([_meta(I31 // 2 - 1, 'float16')]) == ('int', 'buf')
    assert K._mode([_meta(I31 // 2, 'float16')]) == ('int', 'ptr')
    assert K._mode([_meta(I31 - 1, 'float16')]) == ('long long', 'ptr')
    src = K.source('int', 'buf')
    assert 'const int s_qb = (int)s_q * 2;' in src and '* 2u;' in src and 'typedef _Float16 T;' in src


# --- GPU ------------------------------------------------------------------------------------------------------------
# rows longer than a wave whose odd length puts every second row on a 2-byte, not a 4-byte, boundary; (2, 2): the
# smallest periodic wrap
GPU_LATTICES = {
    'D2Q9-srt-periodic-fzyx': Lattice('D2Q9', (7, 66)),
    'D2Q9-srt-wrap-aos': Lattice('D2Q9', (2, 2), compressible=False, layout='numpy'),
    'D2Q9-trt-channel-aos': Lattice('D2Q9', (7, 66), 'trt', False, walls='channel', layout='numpy'),
    'D2Q9-srt-cavity-fzyx': Lattice('D2Q9', (7, 66), walls='cavity'),
    'D2Q9-mrt-periodic-guo': Lattice('D2Q9', (7, 66), 'mrt', True, 'guo'),
    'D3Q19-srt-channel-guo-fzyx': Lattice('D3Q19', (5, 6, 67), 'srt', False, 'guo', walls='channel'),
    'D3Q19-trt-periodic-aos': Lattice('D3Q19', (5, 6, 67), 'trt', True, layout='numpy'),
    'D3Q19-mrt-channel-fzyx': Lattice('D3Q19', (5, 6, 67), 'mrt', True, walls='channel'),
}


def run_gpu(step, x0, g):
    """One step and one adjoint step on the step's own arrays: (result, gradient) as float64."""
    import torch
    step.set_pdfs(torch.tensor(x0, dtype=torch.float16, device='cuda'))
    step.run(1, record=True)
    out = step.pdf_array.double().cpu().numpy()
    step.set_adjoint_pdfs(torch.tensor(g, dtype=torch.float16, device='cuda'))
    step.run_backward(1)
    torch.cuda.synchronize()
    return out, step.adjoint_pdf_array.double().cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('zc', [False, True], ids=['plain', 'zero-centred'])
@pytest.mark.parametrize('name', list(GPU_LATTICES))
def test_fp16_lattice_gpu_one_step(name, zc, monkeypatch):
    """The HIP kernels (``_Float16`` storage, 2-byte buffer accesses): one step and one adjoint step inside the
    one-step bound."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    lat = GPU_LATTICES[name]
    step = lat.step('float16', zc, 'gpu')
    assert step._lattice is not None
    x0, g, ref, gref = one_step_reference(GPU_LATTICES, name, zc)
    out, grad = run_gpu(step, x0, g)
    assert step.pdf_array.dtype == torch.float16
    fns = set(step._lattice_kernels()._fns)
    assert {k[0] for k in fns} == {'fwd', 'adj'} and all(k[1:3] == ('int', 'buf') for k in fns), fns
    wf, wg = worst(out, ref), worst(grad, gref)
    print(f'{name} zero_centered={zc}: forward {wf:.3f}, adjoint {wg:.3f} of the bound')
    assert wf <= 1.0 and wg <= 1.0
    if lat.wall is not None:
        assert np.array_equal(out[lat.wall], x0[lat.wall]) and np.array_equal(grad[lat.wall], g[lat.wall])


@pytest.mark.gpu
@pytest.mark.parametrize('zc', [False, True], ids=['plain', 'zero-centred'])
def test_fp16_lattice_ptr_addressing_gpu(zc, monkeypatch):
    """``PSAD_LBM_ADDR=ptr``: plain ``_Float16`` pointers instead of buffer resources, the same bound."""
    monkeypatch.setenv('PSAD_LBM_ADDR', 'ptr')
    name = 'D3Q19-srt-channel-guo-fzyx'
    step = GPU_LATTICES[name].step('float16', zc, 'gpu')
    x0, g, ref, gref = one_step_reference(GPU_LATTICES, name, zc)
    out, grad = run_gpu(step, x0, g)
    fns = set(step._lattice_kernels()._fns)
    assert fns and all(k[1:3] == ('int', 'ptr') for k in fns), fns
    wf, wg = worst(out, ref), worst(grad, gref)
    print(f'{name} ptr zero_centered={zc}: forward {wf:.3f}, adjoint {wg:.3f} of the bound')
    assert wf <= 1.0 and wg <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('zc', [False, True], ids=['plain', 'zero-centred'])
@pytest.mark.parametrize('name', ['D2Q9-srt-periodic-fzyx', 'D2Q9-srt-wrap-aos', 'D2Q9-trt-channel-aos',
                                  'D2Q9-srt-cavity-fzyx', 'D2Q9-mrt-periodic-guo', 'D3Q19-srt-channel-guo-fzyx',
                                  'D3Q19-trt-periodic-aos', 'D3Q19-mrt-channel-fzyx'])
def test_fp16_timestep_op_gpu(name, zc, monkeypatch):
    """T = 3 through ``create_timestep_op`` (the states between in the op's row-interleaved float16 arrays): float16
    out and gradient, the error against the float64 chain at most 4× the float32 chain's."""
    import torch
    monkeypatch.delenv('PSAD_LBM_ADDR', raising=False)
    lat = GPU_LATTICES[name]
    x0, g, ref64, ref32 = three_step_reference(lat, zc)
    step = lat.step('float16', zc, 'gpu')
    x = step.empty_pdfs()
    x.copy_(torch.tensor(x0, dtype=torch.float16, device='cuda'))
    x.requires_grad_(True)
    out = step.create_timestep_op(3).apply(x)
    out.backward(torch.tensor(g, dtype=torch.float16, device='cuda'))
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and x.grad.dtype == torch.float16
    check_three_steps(f'{name} zero_centered={zc}', out.detach().double().cpu().numpy(), x.grad.double().cpu().numpy(),
                      ref64, ref32)
