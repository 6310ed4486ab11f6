"""Generate ``tests/golden/emit_source_sha.json`` (run: python tests/golden/make_emit_golden.py): the SHA-256 of every
HIP source the stencil emitter (``backends/hip_emitter``, ``backends/hip_band``) prints, over three sets of rows.
No GPU and no compile: the sources are text. ``tests/test_emit_golden.py`` compares ``rows()`` with the JSON, so
"no hash moved" means that a change of the emitter left every code object, and with it behaviour and speed, alone.

1. plan rows — every launch plan ``HipStencilKernel._plan_march`` returns over the matrix of
   ``make_march_plan_golden.py`` (its kernels, stand-in tensors and environment; imported, not copied): the source of
   ``hk.source(plan.variant)``, each distinct (kernel, variant) once, keyed ``<kernel> | <variant>``;
2. the default plans of the benchmark shapes (1024³, 768³, 512³, 511³, 510³, 255³, 4096², the slabs …) for both
   boundary modes, forward and adjoint, at pointer alignments 256 and 4, where set 1 lacks them;
3. ``EXPLICIT`` — direct calls of the emit functions for what no plan reaches: ``emit_pointwise``,
   ``emit_zero_border``, every ``emit_generic`` form, and the ``MarchConfig`` knobs the plans leave at their defaults.

A source that raises is recorded as ``ERROR <type>: <message>``.

``python scripts/emit_coverage.py`` runs ``rows()`` and the periodic rows of ``tests/test_periodic_march.py`` under a
line collector: every statement of the emitter files (the ``hip_emitter`` and ``hip_band`` packages) is executed except
``raise`` statements. When these rows were first generated, before any line of the emitter changed,
the collector also left six statements in four places that no ``MarchConfig`` enters; they are deleted (every hash
unchanged):

* ``_ws_piece_offsets(with_lds=True)`` (the ``lo_<field>`` LDS offsets): no caller passed it;
* ``emit_zsum``'s tail for a register-prefetch depth ``PD`` above 1 (the ``if i:`` guard around the second register
  set's loads and the ``break`` between unrolled planes): ``PD = 1`` stood directly above the loop;
* ``rest_block``'s ``continue`` for a cell without centre-plane terms: every cell has the same terms, and a kernel
  without any returns before the loop;
* ``band_plans``' check that a linear term reads the one stencil field at component 0: ``zsum_plan`` only puts
  stencil-field taps there, there is one stencil field, and vector fields have returned before.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import sympy as sp  # noqa: E402

import make_march_plan_golden as G  # noqa: E402
from pystencils_autodiff_amd import AutoDiffOp, ps, workloads as W  # noqa: E402
from pystencils_autodiff_amd.backends import hip_band as B, hip_emitter as E  # noqa: E402
from pystencils_autodiff_amd.backends.kernel_ir import StencilKernel  # noqa: E402

PATH = os.path.join(HERE, 'emit_source_sha.json')


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def attempt(fn):
    """The hash of the source ``fn()`` returns (a string, or a tuple that starts with one), or the error row."""
    try:
        src = fn()
    except Exception as exc:  # noqa: BLE001
        return f'ERROR {type(exc).__name__}: {exc}'
    return sha(src if isinstance(src, str) else src[0])


def variant_text(v):
    return f'march {G.cfg_text(v[1])}' if v[0] == 'march' else ' '.join(v)


def kernel_text(hk):
    """The kernels of the plan matrix share function names across boundary modes and number formats."""
    return f"{hk.name} {'zeros' if hk.ir.zeros else 'None'} {hk.ir.fields[0].dtype.numpy_dtype.name}"


def plan_variants():
    """``{(kernel text, variant text): (kernel, variant)}`` of sets 1 and 2, in the order the plans are made."""
    seen = {}
    planner = G.StubKernel._plan_march

    def recording(self, *args):
        plan = planner(self, *args)
        seen.setdefault((kernel_text(self), variant_text(plan.variant)), (self, plan.variant))
        return plan
    G.StubKernel._plan_march = recording
    try:
        G.rows()
        with G.environment():
            for hk, shapes in G.kernels().values():
                if hk.schedule() == 'march':
                    for shape in shapes:
                        for align in (256, 4):
                            G.plan_row(hk, G.fake_tensors(hk, shape, align), [], shape)
    finally:
        G.StubKernel._plan_march = planner
    return seen


def rows():
    """``{key: sha256 or error text}``."""
    out = {f'{kname} | {vtext}': attempt(lambda: hk.source(variant))
           for (kname, vtext), (hk, variant) in plan_variants().items()}
    for key, fn in explicit_rows():
        assert key not in out, key
        out[key] = attempt(fn)
    return out


def _ir(assignments, name, bh='zeros', **kw):
    return StencilKernel(assignments, boundary_handling=bh, function_name=name, target='gpu', **kw).ir


def _ac(pairs):
    return ps.AssignmentCollection(dict(pairs))


def _kernels():
    """The small kernels of the explicit rows, name → KernelIR."""
    K = {}
    for dts in ('float32', 'float16', 'float64'):
        a, b, o = ps.fields(f'a, b, o: {dts}[3d]')
        s = sp.Symbol('s')
        K[f'axpy_{dts}'] = _ir(_ac({o.center: s * a.center + b.center}), 'axpy')
        u, o = ps.fields(f'u, o: {dts}[3d]')
        # nonlinear in an off-centre plane (the plane ring), a point field, an integer power
        K[f'ring_pt_{dts}'] = _ir(_ac({o.center: u[1, 0, 0] * u[-1, 0, 0] + u[0, 1, 1] ** 2 + b.center * u[0, 0, -1]}),
                                  'ring_pt')
        # linear off the centre plane, a centre-plane remainder that reads a point field
        K[f'lin_pt_{dts}'] = _ir(_ac({o.center: u[1, 0, 0] + u[-1, 0, 0] + 0.5 * u[0, 0, 1] + b.center * u.center}),
                                 'lin_pt')
        K[f'lin_b_{dts}'] = _ir(_ac({o.center: u[1, 0, 0] + u[-1, 0, 0] + 0.5 * u[0, 0, 1] + b.center}), 'lin_b')
        v = ps.fields(f'v: {dts}[3d]')
        K[f'two_{dts}'] = _ir(_ac({o.center: u[1, 0, 0] + u[-1, 0, 0] + 0.5 * u[0, 0, 1] + 0.25 * u[0, 1, -1] +
                                   v[0, -1, 0] + 2 * v[0, 0, 1] + v[1, 0, 0]}), 'two')
        K[f'sq_{dts}'] = _ir(_ac({o.center: u[1, 0, 0] + u[0, 0, -1] + u.center ** 2}), 'sq')
        p, q = ps.fields(f'p, q: {dts}[3d]')
        K[f'three_{dts}'] = _ir(_ac({o.center: u[1, 0, 0], p.center: u[0, 1, 0], q.center: u[0, 0, 1]}), 'three')
        K[f'flat_{dts}'] = _ir(_ac({o.center: u[0, 1, 0] + u[0, -1, 0] + 0.5 * u[0, 0, 1] + 0.25 * u[0, 0, -1]}), 'flat')
    for name, builder in (('diffusion7', W.diffusion_7pt), ('stencil27_f32', lambda: W.stencil_27pt(dtype='float32')),
                          ('stencil27', W.stencil_27pt), ('varcoef', W.varcoef_diffusion_7pt),
                          ('varcoef_f16', lambda: W.varcoef_diffusion_7pt(dtype='float16')),
                          ('veclap', W.vector_laplace_7pt), ('veclap_f16', lambda: W.vector_laplace_7pt(dtype='float16')),
                          ('laplace5', W.laplace_5pt), ('adv3', lambda: G._advection3d('float32'))):
        K[name] = _ir(AutoDiffOp(builder(), boundary_handling='zeros').forward_assignments, name)
    u, o = ps.fields('u, o: float32[3d]')
    K['exp'] = _ir(_ac({o.center: sp.exp(u[1, 0, 0]) * u[-1, 0, 0]}), 'exp')
    K['periodic'] = _ir(_ac({o.center: u[1, 0, 0] + u[0, -1, 0] + u[0, 0, 2]}), 'periodic', bh='periodic')
    K['push'] = _ir(_ac({o[1, 0, 0]: u.center, o[0, -1, 0]: 2 * u.center}), 'push')
    K['push_periodic'] = _ir(_ac({o[1, 0, 0]: u.center}), 'push_periodic', bh='periodic')
    K['strided'] = _ir(_ac({o.center: u[1, 0, 0] + u.center}), 'strided', bh=None,
                       iteration_slice=(slice(1, -1, 2), slice(1, -1), slice(2, -1, 3)))
    u1, o1 = ps.fields('u, o: float32[1d]')
    K['line'] = _ir(_ac({o1.center: u1[1] + u1[-1]}), 'line')
    t, o = ps.fields('t(2, 2), o: float32[3d]')
    K['tensor'] = _ir(_ac({o.center: t[1, 0, 0](0, 1) * t[-1, 0, 0](1, 0) + t[0, 1, 0](1, 1)}), 'tensor')
    return K


def _band_plan_rows():
    """The band knobs through the planner (it sets ``BX``, ``BMASK`` … for the row length): 27-point kernels whose
    overrides carry one knob each, on rows of whole chunks, of a partial last chunk and on half dwords. A knob that
    does not apply to a row length (``BREG``, ``BZF``, ``BTAIL`` on rows of whole chunks …) prints the default source:
    that row pins only that the knob changes nothing there."""
    out = []
    knobs = [dict(BEDGE=0), dict(BNT=0), dict(BREG=1), dict(BZF=0), dict(BPAD=1), dict(BTAIL=0), dict(BFREE=1),
             dict(BFREE=2), dict(BTRIM=1), dict(BTRIM=2), dict(MAP=1), dict(BPAD=1, BTRIM=2), dict(BZF=0, BTAIL=0)]
    cases = [(f'stencil27{sfx}', lambda d=d: W.stencil_27pt(dtype=d), knob, babl)
             for sfx, d in (('', 'float16'), ('_f32', 'float32'))
             for knob, babl in [(k, 0) for k in knobs] + [(dict(), b) for b in (1, 2, 3)]]
    launches = [(shape, opt) for shape in ((16, 32, 256), (16, 32, 255), (16, 32, 262), (20, 24, 256))
                for opt in (dict(), dict(start_signal=True, halo_wait=True, z_range=(3, 13)))]
    cases = [(name, builder, 'zeros', knob, babl, launches) for name, builder, knob, babl in cases]
    cases += [('diffusion7_f16', lambda: W.diffusion_7pt(dtype='float16'), 'zeros', dict(BTRIM=2), 0, launches),
              ('varcoef', W.varcoef_diffusion_7pt, 'zeros', dict(WS=1, NW=8, CX=2, WX=2, NR=1, D=2), 3, launches)]
    # interior-only kernels: masked stores, zeros over the x border, rows whose tail is one dword; bands past yhi
    border = [((16, 32, X), opt) for X in (256, 255, 257, 258, 262) for opt in (dict(), dict(x_border=True))]
    cases += [('stencil27', W.stencil_27pt, None, dict(), 0, border),
              ('stencil27_f32', lambda: W.stencil_27pt(dtype='float32'), None, dict(), 0, border),
              ('stencil27', W.stencil_27pt, 'zeros', dict(), 0, [((16, 30, 256), dict()), ((16, 30, 262), dict())])]
    for name, builder, bh, knob, babl, todo in cases:
        tun = knob if name == 'varcoef' else dict(BAND=4, **knob)
        op = AutoDiffOp(builder(), boundary_handling=bh)
        hk = G.StubKernel(StencilKernel(op.forward_assignments, boundary_handling=bh, function_name=name,
                                        target='gpu', gpu_indexing_params=tun))
        for shape, opt in todo:
            def source(hk=hk, shape=shape, opt=opt, babl=babl):
                G.HK.PROBE_KNOBS.clear()
                if babl:
                    G.HK.PROBE_KNOBS['BABL'] = babl
                try:
                    with G.environment():
                        plan = hk._plan_march(G.fake_tensors(hk, shape, 256), [], shape, 0, opt.get('z_range'),
                                              opt.get('x_border', False), None, opt.get('start_signal', False),
                                              opt.get('halo_wait', False))
                finally:
                    G.HK.PROBE_KNOBS.clear()
                return hk.source(plan.variant)
            out.append((f'planned {name} {bh} {G.kv_text(tun)} BABL={babl} {G.shape_text(shape)} {G.kv_text(opt)}', source))
    return out


def pointwise_plain_loads(ir):
    """``emit_pointwise`` with the module switch ``POINTWISE_NT_LOAD`` off (``scripts/tune_march.py`` sets it)."""
    saved, E.pointwise.POINTWISE_NT_LOAD = E.pointwise.POINTWISE_NT_LOAD, False
    try:
        return E.emit_pointwise(ir, 'axpy')
    finally:
        E.pointwise.POINTWISE_NT_LOAD = saved


def explicit_rows():
    """``[(key, function that returns the source)]`` of set 3."""
    K = _kernels()
    M = E.MarchConfig
    out = []

    def row(fn, kname, **kw):
        out.append((f'{fn.__name__} {kname} {G.kv_text(kw)}'.rstrip(), lambda: fn(K[kname], kname, **kw)))

    def march(fn, kname, **cfg):
        out.append((f'{fn.__name__} {kname} {G.kv_text(cfg)}', lambda: fn(K[kname], kname, M(**cfg))))
    for dts in ('float32', 'float16', 'float64'):
        row(E.emit_pointwise, f'axpy_{dts}')
    out.append(('emit_pointwise axpy_float32 POINTWISE_NT_LOAD=False', lambda: pointwise_plain_loads(K['axpy_float32'])))
    for esize in (2, 4, 8):
        for idx32 in (False, True):
            out.append((f'emit_zero_border {esize} idx32={idx32}', lambda e=esize, i=idx32: E.emit_zero_border(e, i)))
    for kname in ('veclap', 'tensor', 'periodic', 'push', 'push_periodic', 'strided', 'line', 'adv3'):
        for idx32 in (False, True):
            for contig in (False, True):
                for shared in (False, True):
                    row(E.emit_generic, kname, idx32=idx32, contig=contig, shared=shared)
    # the register-prefetch plane ring: two planes in flight, point fields, pairs, non-temporal stores, no fast path
    for kname, ve in (('varcoef', 4), ('ring_pt_float32', 4), ('ring_pt_float16', 8), ('varcoef_f16', 8)):
        for cfg in (dict(PD=2), dict(NT_STORE=True), dict(PR=1), dict(PR=1, SFAST=0), dict(PR=1, NT_STORE=True),
                    dict(PR=1, PD=2), dict(WS=True), dict(WS=True, PR=1), dict(WS=True, PR=1, NT_STORE=True),
                    dict(WS=True, SFAST=0), dict(WS=True, BABL=3), dict(MAP=1, SIG=True), dict(NW=1, CX=1)):
            march(E.emit_march, kname, VE=ve, **cfg)
    for kname in ('veclap', 'veclap_f16', 'adv3'):
        for cfg in (dict(WS=True), dict(WS=True, PR=1), dict(WS=True, PR=1, NT_STORE=True), dict(WS=True, NW=8, NR=1)):
            march(E.emit_march, kname, VE=4 if kname != 'veclap_f16' else 8, **cfg)
    # what emit_march refuses, and the geometries that do not apply
    for kname, cfg in (('line', dict()), ('exp', dict(PR=1)), ('varcoef', dict(PR=1, CX=1)),
                       ('ring_pt_float64', dict(VE=2, PR=1)), ('veclap', dict()), ('tensor', dict(WS=True)),
                       ('axpy_float32', dict(WS=True)), ('exp', dict(WS=True))):
        march(E.emit_march, kname, **cfg)
    # zsum: pairs without the inline-asm reads, remainders that read point fields, zeros outside the x range
    for kname, ve in (('diffusion7', 4), ('stencil27_f32', 4), ('lin_pt_float32', 4), ('lin_b_float32', 4),
                      ('lin_pt_float16', 8), ('lin_b_float16', 8), ('veclap', 4), ('laplace5', 4), ('flat_float32', 4),
                      ('two_float32', 4), ('lin_pt_float64', 2)):
        for cfg in (dict(), dict(PK=True), dict(PK=True, AR=True), dict(XB=True), dict(PK=True, XB=True, NT_STORE=True),
                    dict(WS=True), dict(WS=True, PK=True, AR=True, XB=True), dict(WS=True, XM=True, HWAIT=True),
                    dict(WS=True, CX=4, D=2), dict(NW=2, CX=4, WX=2, NR=1)):
            march(E.emit_zsum, kname, VE=ve, ZSUM=True, **cfg)
    for kname in ('line', 'push', 'exp', 'varcoef'):
        march(E.emit_zsum, kname, ZSUM=True)
    # the half ring: rows on odd pitches and half dwords, one and two stencil fields, no z radius
    for kname in ('stencil27', 'two_float16', 'flat_float16', 'veclap_f16', 'lin_b_float16'):
        for cfg in (dict(), dict(XM=True), dict(XM=True, XO=1), dict(XM=True, XO=2), dict(XB=True, NT_STORE=True),
                    dict(XM=True, XO=1, XB=True, CX=8, NR=1)):
            march(E.emit_zsum, kname, **{**dict(VE=8, ZSUM=True, WS=True, CX=4), **cfg})
    # the band schedule on kernels it does not take
    for kname in ('lin_b_float16', 'lin_pt_float16', 'veclap_f16', 'two_float16', 'varcoef_f16', 'axpy_float16',
                  'lin_pt_float64', 'sq_float16', 'three_float16'):
        march(B.emit_band, kname, VE=8, BAND=4, BX=256)
    return out + _band_plan_rows()


def encode(table):
    return '{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in table.items()) + '\n}\n'


if __name__ == '__main__':
    table = rows()
    with open(PATH, 'w') as fh:
        fh.write(encode(table))
    errors = [k for k, v in table.items() if v.startswith('ERROR')]
    print(f'{len(table)} rows, {len(set(table.values()))} distinct, {len(errors)} errors, '
          f'{os.path.getsize(PATH)} bytes -> {PATH}')
    for k in errors:
        print(f'  {k}: {table[k]}')
