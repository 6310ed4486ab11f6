"""Generate ``tests/golden/march_plan.json`` (run: python tests/golden/make_march_plan_golden.py): what the march
planner decides, over a matrix of kernels, shapes, vector widths, tile overrides, environment switches, pointer
alignments and launch options. No GPU: the planner is host code; compile and residency are stubbed (``function`` and
``_resident_slots`` return None). ``make_emit_golden.py`` pins the emitted source of every plan made here.

Two kinds of rows, both entered only through names that keep their signature:

* config rows — ``hip_kernel.default_march_config(ir, ve, shape, tuning, band=)``: the ``MarchConfig`` fields that
  differ from the dataclass defaults, or ``ERROR <type>: <message>``;
* plan rows — ``HipStencilKernel._plan_march(tensors, halo_list, shape, device, z_range, x_border, z_limits,
  start_signal, halo_wait)``: variant, grid, block, argument kinds, static arguments and the signal / wait offsets.

The JSON keeps every distinct value once (``values``) and maps ``rows[kernel][key]`` to its index (``encode``).
``tests/test_march_plan.py`` compares ``rows()`` with it.
"""
import contextlib
import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import sympy as sp  # noqa: E402
import torch  # noqa: E402

from pystencils_autodiff_amd import AutoDiffOp, ps, workloads as W  # noqa: E402
from pystencils_autodiff_amd.backends import hip_kernel as HK  # noqa: E402
from pystencils_autodiff_amd.backends.hip_emitter import MarchConfig  # noqa: E402
from pystencils_autodiff_amd.backends.kernel_ir import StencilKernel  # noqa: E402

PATH = os.path.join(HERE, 'march_plan.json')
ENV_KEYS = ('PSAD_MARCH', 'PSAD_BAND', 'PSAD_BAND_UNALIGNED', 'PSAD_XO', 'PSAD_MARCH_ZC', 'PSAD_MARCH_BLOCKS')


class FakeTensor:
    """What ``_plan_march`` reads of a tensor: pointer, shape, dtype, contiguity."""
    is_cuda = True

    def __init__(self, shape, dtype, ptr):
        self.shape, self.dtype, self._ptr = tuple(shape), dtype, ptr

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return True

    def stride(self):
        st, acc = [], 1
        for s in reversed(self.shape):
            st.append(acc)
            acc *= s
        return tuple(reversed(st))

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n


class StubKernel(HK.HipStencilKernel):
    """The planner without a GPU: no compile, no residency query."""

    def function(self, variant, device):
        return None

    def _resident_slots(self, fn, block, device):
        return None


def _varcoef2d(dts):
    u, k, out = ps.fields(f'u, k, out: {dts}[2d]')
    nb = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    return ps.AssignmentCollection({out.center: u.center + 0.1 * sp.Add(
        *[sp.Rational(1, 2) * (k.center + k[o]) * (u[o] - u.center) for o in nb])})


def _advection3d(dts):
    u, out = ps.fields(f'u(3), out(3): {dts}[3d]')
    e, m = [(1, 0, 0), (0, 1, 0), (0, 0, 1)], [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    return ps.AssignmentCollection({out.center(c): u.center(c) - 0.05 * sp.Add(
        *[u.center(d) * (u[e[d]](c) - u[m[d]](c)) / 2 for d in range(3)]) for c in range(3)})


def _advection2d(dts):
    u, out = ps.fields(f'u(2), out(2): {dts}[2d]')
    e, m = [(1, 0), (0, 1)], [(-1, 0), (0, -1)]
    return ps.AssignmentCollection({out.center(c): u.center(c) - 0.05 * sp.Add(
        *[u.center(d) * (u[e[d]](c) - u[m[d]](c)) / 2 for d in range(2)]) for c in range(2)})


def _wide(radius, dts):
    """Products of taps ``radius`` cells out on three fields: plane rings too large for the LDS."""
    a, b, c, o = ps.fields(f'a, b, c, o: {dts}[3d]')
    R = radius
    return ps.AssignmentCollection({o.center: a[0, 0, R] * b[0, R, 0] + a[-R, 0, 0] * b[R, -R, 0] +
                                    c[-R, R, -R] * c[R, 0, R] * a[0, -R, 0]})


# (name, builder, the benchmark shapes of this kernel)
CASES = [
    ('diffusion7', W.diffusion_7pt, [(1024,) * 3, (512,) * 3, (768,) * 3, (128, 1024, 1024), (255,) * 3, (64, 300, 261)]),
    ('diffusion7_f16', lambda: W.diffusion_7pt(dtype='float16'), [(768,) * 3, (511,) * 3, (510,) * 3, (512, 512, 520)]),
    ('stencil27', W.stencil_27pt, [(768,) * 3, (1024,) * 3, (512,) * 3, (96, 768, 768), (511,) * 3, (510,) * 3,
                                   (255,) * 3, (512, 512, 1000), (512, 512, 320)]),
    ('laplace5', W.laplace_5pt, [(4096, 4096), (4097, 4097)]),
    ('asym7', W.asym_7pt, [(256,) * 3]),
    ('varcoef', W.varcoef_diffusion_7pt, [(768,) * 3, (512,) * 3]),
    ('varcoef_f16', lambda: W.varcoef_diffusion_7pt(dtype='float16'), [(768,) * 3]),
    ('veclap', W.vector_laplace_7pt, [(384,) * 3]),
    ('diffusion7_f64', lambda: W.diffusion_7pt(dtype='float64'), [(512,) * 3]),
    ('stencil27_f32', lambda: W.stencil_27pt(dtype='float32'), [(768,) * 3]),
    ('varcoef2d', lambda: _varcoef2d('float32'), []),
    ('varcoef2d_f16', lambda: _varcoef2d('float16'), []),
    ('adv3', lambda: _advection3d('float32'), []),
    ('adv3_f16', lambda: _advection3d('float16'), []),
    ('adv2', lambda: _advection2d('float32'), []),
    ('adv2_f16', lambda: _advection2d('float16'), []),
]
COMMON = {3: [None, (33, 40, 64), (16, 32, 256), (16, 32, 255), (16, 32, 262), (96, 768, 768), (1, 1, 1)],
          2: [None, (64, 300), (65, 257), (4096, 4096)]}
TUNING_SHAPES = {3: [(16, 32, 256), (96, 768, 768)], 2: [(64, 300), (4096, 4096)]}
# planes of 2 GiB and more (the LDS-DMA loader's 32-bit offsets)
HUGE = {3: (4, 40000, 40000), 2: (40000, 40000)}

# one row per TILE_KEYS entry at a non-default value (both values of the switches), then the named combinations
TUNINGS = [{'CX': 1}, {'CX': 2}, {'WX': 2}, {'NR': 1}, {'ZMIN': 4}, {'ZMAX': 200}, {'BLK': 300}, {'D': 1}, {'NW': 2},
           {'NT_STORE': 0}, {'ZSUM': 0}, {'ZSUM': 1}, {'PK': 0}, {'PK': 1}, {'WS': 0}, {'WS': 1}, {'AR': 0},
           {'VIEW2D': 'zy'}, {'ZC': 5}, {'BLOCKS': 100}, {'MAP': 1}, {'BAND': 2}, {'BAND': 4},
           {'BAND': 0}, {'BTY': 16}, {'BTRIM': 1}, {'BEDGE': 0}, {'BPAD': 0}, {'BPAD': 1}, {'BZF': 0}, {'BREG': 1},
           {'BNT': 0}, {'BFREE': 1}, {'BTAIL': 0}, {'SFAST': 0}, {'SLP': 1}, {'PR': 1}, {'PD': 2},
           {'block_size': 8}, {'BOGUS': 1}, {'NW': 3}, {'NW': 8}, {'BAND': 4, 'BTY': 6},
           {'BTRIM': 3, 'ZMIN': 8, 'ZMAX': 16}, {'BTRIM': 3, 'ZMIN': 8}, {'BAND': 4, 'BTY': 16, 'D': 1},
           {'WS': 1, 'NW': 8, 'CX': 2, 'WX': 2, 'NR': 1, 'D': 2}, {'WS': 1, 'CX': 4, 'NR': 8, 'D': 6}, {'CX': 8, 'NR': 8}]
ALIGNS = (256, 16, 8, 4, 2)


def kernels():
    """name → StubKernel, for both boundary modes, forward and adjoint."""
    out = {}
    for name, builder, shapes in CASES:
        for bh in ('zeros', None):
            op = AutoDiffOp(builder(), boundary_handling=bh)
            for which, asg in (('fwd', op.forward_assignments), ('bwd', op.backward_assignments)):
                hk = StubKernel(StencilKernel(asg, boundary_handling=bh, function_name=f'{name}_{which}', target='gpu'))
                out[f'{name}/{bh}/{which}'] = (hk, shapes)
    return out


@contextlib.contextmanager
def environment(**env):
    """The planner's environment switches: exactly ``env`` set, the others unset; restored afterwards."""
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


DEFAULTS = {f.name: f.default for f in dataclasses.fields(MarchConfig)}


def cfg_text(cfg):
    return ','.join(f'{k}={v}' for k, v in cfg.__dict__.items() if DEFAULTS[k] != v) or 'defaults'


def kv_text(d):
    return ','.join(f'{k}={v}' for k, v in d.items()).replace(' ', '')


def shape_text(shape):
    return 'x'.join(str(n) for n in shape) if shape is not None else 'None'


def runs_text(items):
    """'ptr ptr ptr i32' → 'ptr*3 i32'."""
    out = []
    for it in items:
        if out and out[-1][0] == it:
            out[-1][1] += 1
        else:
            out.append([it, 1])
    return ' '.join(f'{it}*{n}' if n > 1 else it for it, n in out)


def config_row(hk, ve, shape, tuning, band):
    try:
        return cfg_text(HK.default_march_config(hk.ir, ve, shape, tuning, band=band))
    except Exception as exc:  # noqa: BLE001
        return f'ERROR {type(exc).__name__}: {exc}'


def plan_row(hk, tensors, halos, shape, z_range=None, x_border=False, z_limits=None, start_signal=False,
             halo_wait=False):
    try:
        plan = hk._plan_march(tensors, halos, shape, 0, z_range, x_border, z_limits, start_signal, halo_wait)
    except Exception as exc:  # noqa: BLE001
        return f'ERROR {type(exc).__name__}: {exc}'
    v = plan.variant
    variant = f'march {cfg_text(v[1])}' if v[0] == 'march' else ' '.join(v)
    return (f'{variant} | grid={plan.grid} block={plan.block} | {runs_text(plan.kinds)} | '
            f'{" ".join(str(s) for s in plan.statics)} | sig={plan.sig_offsets} hwait={plan.hwait_offsets}')


def vector_widths(hk):
    ve = hk._vec_elems()
    return [v for v in dict.fromkeys((ve, ve // 2, ve // 4, 1)) if v >= 1]


def fake_tensors(hk, shape, align_in, align_out=None):
    written = {f.name for f in hk.ir.fields_written}
    return [FakeTensor(tuple(shape) + tuple(f.index_shape), getattr(torch, f.dtype.numpy_dtype.name),
                       (1 << 32) + (align_out if align_out and f.name in written else align_in)) for f in hk.ir.fields]


def real_tensors(hk, shape, offset, halo_planes):
    """CPU tensors sliced out of flat buffers at an element offset (the halo checks want real tensors): the field
    tensors, and per stencil field a (lo, hi) pair of halo tensors (``halo_planes`` = 'both', 'hi' or 'short')."""
    def make(shp, f):
        n = 1
        for s in tuple(shp) + tuple(f.index_shape):
            n *= s
        flat = torch.zeros(n + 8, dtype=getattr(torch, f.dtype.numpy_dtype.name))
        return flat[offset:offset + n].view(tuple(shp) + tuple(f.index_shape))
    tensors = [make(shape, f) for f in hk.ir.fields]
    halos = []
    for f in hk.ir.stencil_fields:
        hshape = ((2,) + tuple(shape[1:])) if halo_planes != 'short' else (1,) + tuple(shape[1:-1]) + (shape[-1] // 2,)
        halos += [None if halo_planes == 'hi' else make(hshape, f), make(hshape, f)]
    return tensors, halos


def align_text(tensors, halos=()):
    return 'a' + ''.join(str(HK._align_class(t.data_ptr())) if t is not None else '-' for t in list(tensors) + list(halos))


def rows():
    """``{kernel: {key: value}}`` over the whole matrix."""
    out = {}
    saved_knobs = dict(HK.PROBE_KNOBS)
    HK.PROBE_KNOBS.clear()
    try:
        with environment():
            for kname, (hk, shapes) in kernels().items():
                out[kname] = _kernel_rows(kname, hk, shapes)
            out.update(_extra_rows())
        out = {kname: {key.rstrip(): val for key, val in kr.items()} for kname, kr in out.items()}
    finally:
        HK.PROBE_KNOBS.clear()
        HK.PROBE_KNOBS.update(saved_knobs)
    return out


# kernels (forward, 'zeros') whose overrides are crossed with TUNINGS, those that also take them through PSAD_MARCH,
# and those that get the launch options, mixed alignments and halo planes
TUNED = ('diffusion7', 'stencil27', 'varcoef_f16', 'varcoef2d_f16', 'adv3_f16')
TUNED_ENV = ('stencil27', 'varcoef2d_f16')
OPTIONS = ('diffusion7', 'diffusion7_f16', 'stencil27', 'laplace5', 'varcoef', 'varcoef_f16', 'veclap', 'varcoef2d_f16',
           'adv3_f16', 'adv2')


def _kernel_rows(kname, hk, shapes):
    if hk.schedule() != 'march':
        return {'schedule': hk.schedule()}
    r = {}
    name, bh, which = kname.split('/')
    nd = hk.ir.ndim
    zeros, first = bh == 'zeros', (bh, which) == ('zeros', 'fwd')
    small = [s for s in COMMON[nd] if s is not None]
    if first:
        _config_rows(r, hk, shapes + COMMON[nd], small[:4])
    else:
        _config_rows(r, hk, (shapes + [None] + small[:3]) if zeros else (shapes[:1] + small[1:2]), [])
    if first and name in TUNED:
        _override_rows(r, hk, hk._vec_elems(), TUNING_SHAPES[nd], name in TUNED_ENV)
    # ---- plan rows: stand-in tensors of every alignment class, default launches
    for shape in (shapes + small[:4] + [HUGE[nd]]) if first else (shapes + small[1:3]) if zeros else (shapes[:1] + small[1:2]):
        for align in ALIGNS if first and shape in small else (256, 4) if shape != HUGE[nd] else (256,):
            ts = fake_tensors(hk, shape, align)
            r[f'plan {shape_text(shape)} {align_text(ts)}'] = plan_row(hk, ts, [], shape)
    if first and name in OPTIONS:
        for a_in, a_out in ((256, 4), (4, 256), (16, 2), (8, 16)):
            ts = fake_tensors(hk, small[1], a_in, a_out)
            r[f'plan {shape_text(small[1])} {align_text(ts)}'] = plan_row(hk, ts, [], small[1])
        _option_rows(r, hk, small[1:3] if nd == 3 else [small[0], small[2]], HUGE[nd])
        _halo_rows(r, hk, (16, 32, 256) if nd == 3 else (16, 1024))
    elif which == 'fwd' and not zeros:         # (interior-only bounds: what x_border and z_limits change)
        ts = fake_tensors(hk, small[1], 256)
        for opt in (dict(x_border=True), dict(x_border=True, z_limits=(1, 15)), dict(z_limits=(2, 9), z_range=(0, 5))):
            r[f'plan {shape_text(small[1])} {align_text(ts)} {kv_text(opt)}'] = plan_row(hk, ts, [], small[1], **opt)
    return r


def _config_rows(r, hk, shapes, narrow):
    """Shapes × band on / off at the full vector width, no overrides; on the ``narrow`` shapes also the narrower
    vectors (which the vector search asks for without the band)."""
    full = hk._vec_elems()
    for shape in shapes:
        for ve in vector_widths(hk) if shape in narrow else [full]:
            for band in (1, 0) if ve == full else (0,):
                r[f'cfg {shape_text(shape)} v{ve} b{band}'] = config_row(hk, ve, shape, None, bool(band))


def _override_rows(r, hk, ve, shapes, through_env):
    """Overrides through the tuning dict (and ``PSAD_MARCH``), ``PSAD_BAND=0`` and the probe knob, on two shapes."""
    for shape in shapes:
        for tun in TUNINGS:
            as_dict = {'block_size': (8, 4, 2)} if 'block_size' in tun else tun
            r[f'cfg {shape_text(shape)} v{ve} b1 {kv_text(tun)}'] = config_row(hk, ve, shape, as_dict, True)
            if through_env:
                with environment(PSAD_MARCH=kv_text(tun)):
                    r[f'cfg {shape_text(shape)} v{ve} b1 PSAD_MARCH={kv_text(tun)}'] = config_row(hk, ve, shape, None, True)
        with environment(PSAD_BAND='0'):
            r[f'cfg {shape_text(shape)} v{ve} b1 PSAD_BAND=0'] = config_row(hk, ve, shape, None, True)
            r[f'cfg {shape_text(shape)} v{ve} b1 BAND=4 PSAD_BAND=0'] = config_row(hk, ve, shape, {'BAND': 4}, True)
        with environment(PSAD_MARCH='CX=2'):       # both sources: the environment wins
            r[f'cfg {shape_text(shape)} v{ve} b1 CX=1,NR=2 PSAD_MARCH=CX=2'] = \
                config_row(hk, ve, shape, {'CX': 1, 'NR': 2}, True)
        HK.PROBE_KNOBS['BABL'] = 2
        try:
            for band in (1, 0):
                r[f'cfg {shape_text(shape)} v{ve} b{band} BABL=2'] = config_row(hk, ve, shape, None, bool(band))
        finally:
            HK.PROBE_KNOBS.clear()


def _option_rows(r, hk, shapes, huge):
    """Launch options and the plan's environment switches."""
    Z = shapes[0][0]
    options = [dict(z_range=(2, 9)), dict(z_range=((0, 2), (Z - 2, Z))), dict(z_range=((0, 2), (Z - 3, Z))),
               dict(z_limits=(1, Z - 1)), dict(z_limits=(1, Z - 1), z_range=(0, 5)), dict(x_border=True),
               dict(x_border=True, z_limits=(1, Z - 1)), dict(start_signal=True), dict(halo_wait=True),
               dict(start_signal=True, halo_wait=True, z_range=(3, Z - 3))]
    for shape, align in [(shapes[0], 256), (shapes[1], 4), (huge, 256)]:
        ts = fake_tensors(hk, shape, align)
        for opt in options if shape != huge else options[:1] + options[3:4]:
            r[f'plan {shape_text(shape)} {align_text(ts)} {kv_text(opt)}'] = plan_row(hk, ts, [], shape, **opt)
    for shape in shapes[1:]:
        for align in (4, 2):
            ts = fake_tensors(hk, shape, align)
            for env in ({'PSAD_BAND_UNALIGNED': '0'}, {'PSAD_XO': '0'}, {'PSAD_BAND': '0'},
                        {'PSAD_BAND_UNALIGNED': '0', 'PSAD_XO': '0'}):
                with environment(**env):
                    r[f'plan {shape_text(shape)} {align_text(ts)} {kv_text(env)}'] = plan_row(hk, ts, [], shape)


def _halo_rows(r, hk, shape):
    """Halo planes: real CPU tensors at element offsets 0, 1, 2."""
    pair = ((0, 2), (shape[0] - 2, shape[0]))
    for offset in (0, 1, 2):
        for planes, opt in (('both', dict()), ('both', dict(z_range=pair, halo_wait=True)), ('hi', dict(z_range=pair)),
                            ('short', dict(z_range=pair)))[:4 if offset == 0 else 2]:
            ts, halos = real_tensors(hk, shape, offset, planes)
            r[f'plan {shape_text(shape)} {align_text(ts, halos)} halos={planes} {kv_text(opt)}'] = \
                plan_row(hk, ts, halos, shape, **opt)


# overrides of kernels whose plane ring does not fit the LDS (the register form, eight waves dropped, the 160 KB error)
WIDE = [('wide3', lambda: _wide(3, 'float32')), ('wide3_f64', lambda: _wide(3, 'float64')),
        ('wide4_f64', lambda: _wide(4, 'float64')), ('wide6_f64', lambda: _wide(6, 'float64'))]
WIDE_TUNINGS = [None, {'WS': 1}, {'WS': 1, 'NW': 8}, {'WS': 1, 'NW': 8, 'WX': 8}, {'WS': 1, 'NW': 8, 'WX': 4, 'NR': 1}]
# a tile or view override on the 2-D row ring of a vector field (back to its zsum plane)
RING_2D_TUNINGS = [{'CX': 2}, {'VIEW2D': 'yx'}, {'NW': 2}, {'WS': 1, 'CX': 2}]
# plans of kernels that carry overrides (``gpu_indexing_params``): builder, overrides, shapes, alignments
TUNED_PLANS = [
    (W.varcoef_diffusion_7pt, dict(WS=1, NW=8, CX=2, WX=2, NR=1, D=2), [(16, 32, 256), HUGE[3]], (256, 4)),
    (lambda: _wide(3, 'float32'), dict(WS=1, NW=8), [(16, 32, 256), HUGE[3]], (256,)),
    (W.stencil_27pt, dict(BAND=4), [(16, 32, 256), (16, 32, 255), (16, 32, 262)], (256, 4, 2)),
    (W.stencil_27pt, dict(BAND=4, BREG=1), [(16, 32, 255), (16, 32, 262)], (256,)),
    (W.diffusion_7pt, dict(ZC=5), [(16, 32, 256), (768,) * 3], (256,)),
    (W.diffusion_7pt, dict(BLOCKS=100), [(16, 32, 256), (768,) * 3], (256,)),
    (W.diffusion_7pt, dict(block_size=(8, 4, 2)), [(16, 32, 256)], (256,)),
    (W.laplace_5pt, dict(VIEW2D='zy'), [(64, 300), (4096, 4096)], (256, 4)),
]


def _extra_rows():
    out = {}
    for name, builder in WIDE:
        op = AutoDiffOp(builder(), boundary_handling='zeros')
        hk = StubKernel(StencilKernel(op.forward_assignments, boundary_handling='zeros', function_name=name, target='gpu'))
        r = out[f'{name}/zeros/fwd'] = {}
        for tun in WIDE_TUNINGS:
            for shape in ((16, 32, 256), None):
                r[f'cfg {shape_text(shape)} v{hk._vec_elems()} b1 {kv_text(tun or {})}'] = \
                    config_row(hk, hk._vec_elems(), shape, tun, True)
    for dts, ve in (('float32', 4), ('float16', 8)):
        op = AutoDiffOp(_advection2d(dts), boundary_handling='zeros')
        hk = StubKernel(StencilKernel(op.forward_assignments, boundary_handling='zeros', function_name='adv2', target='gpu'))
        r = out[f'adv2 {dts} overrides'] = {}
        for tun in RING_2D_TUNINGS:
            for shape in TUNING_SHAPES[2]:
                r[f'cfg {shape_text(shape)} v{ve} b1 {kv_text(tun)}'] = config_row(hk, ve, shape, tun, True)
    r = out['tuned plans'] = {}
    for i, (builder, tun, shapes, aligns) in enumerate(TUNED_PLANS):
        op = AutoDiffOp(builder(), boundary_handling='zeros')
        hk = StubKernel(StencilKernel(op.forward_assignments, boundary_handling='zeros', function_name=f'tuned{i}',
                                      target='gpu', gpu_indexing_params=tun))
        for shape in shapes:
            for align in aligns:
                ts = fake_tensors(hk, shape, align)
                opts = (dict(), dict(halo_wait=True), dict(z_range=(2, 9))) if shape[0] == 16 else (dict(),)
                for opt in opts:
                    r[f'{i} {kv_text(tun)} plan {shape_text(shape)} {align_text(ts)} {kv_text(opt)}'] = \
                        plan_row(hk, ts, [], shape, **opt)
    return out


def encode(table):
    """``rows()`` → the JSON document: distinct values once, ``rows[kernel][first two words of the key][rest]`` → index,
    several to a line."""
    values, index, lines = [], {}, []
    for kname, kr in table.items():
        groups = {}
        for key, val in kr.items():
            words = key.split(' ')
            groups.setdefault(' '.join(words[:2]), {})[' '.join(words[2:])] = index.setdefault(val, len(index))
        lines.append(f'  {json.dumps(kname)}: {{')
        line = '  '
        for gname, g in groups.items():         # flowed: a line break wherever the next piece would pass 118 columns
            pieces = [f'{json.dumps(gname)}: {{'] + [f'{json.dumps(rest)}: {i},' for rest, i in g.items()]
            pieces[-1] = pieces[-1][:-1] + '},'
            for piece in pieces:
                if len(line) + 1 + len(piece) > 118:
                    lines.append(line)
                    line = '  '
                line += ' ' + piece
        lines += [line[:-1], '  },']
    lines[-1] = '  }'
    values = list(index)
    head = ['{', ' "values": ['] + [f'  {json.dumps(v)}' + (',' if i + 1 < len(values) else '') for i, v in enumerate(values)]
    return '\n'.join(head + [' ],', ' "rows": {'] + lines + [' }', '}']) + '\n'


def decode(text):
    doc = json.loads(text)
    return {kname: {f'{gname} {rest}'.rstrip(): doc['values'][i] for gname, g in groups.items() for rest, i in g.items()}
            for kname, groups in doc['rows'].items()}


if __name__ == '__main__':
    table = rows()
    with open(PATH, 'w') as fh:
        fh.write(encode(table))
    print(f'{sum(len(kr) for kr in table.values())} rows, {os.path.getsize(PATH)} bytes -> {PATH}')
