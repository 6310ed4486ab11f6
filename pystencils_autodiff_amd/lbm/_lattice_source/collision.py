"""The collision: the cell's force, its moments, the obstacle cells' copy and the forward cell."""
from .addressing import wrap_lines
from .common import Fa, c_, cFi, cu_poly, feq, mat_row, shift, signed_sum
from . import macroscopic
from .links import cell_density, pull_loads
from .omega import omega_load
from .smagorinsky import smagorinsky_moments
from .solid import forward_blend, solid_load
from .spec import SELF_BIT


def force_loads(cx, L):
    """The cell's force vector and its projections c_i · F (``force_field``)."""
    if not cx.s.ff:
        return
    ct = cx.ct
    fcell = ' + '.join(f'(IDX){a} * f_{a}' for a in cx.axes)
    L.append(f'  const IDX fc = {fcell};')
    for a in range(cx.D):
        L.append(f'  const {ct} F{a} = ({ct})force[(IDX){a} * f_c + fc];')
    for i in range(cx.Q):
        if any(cx.dirs[i]):
            L.append(f'  const {ct} cF{i} = {signed_sum(cx, i, "F")};')


def moments(cx, L):
    """ρ, u (Guo: shifted by F/2 (/ρ)) and what the collision takes besides: u², u·F and 1 − ω/2 (Guo), the TRT
    rates a = (ω₊ + ω₋)/2, b = (ω₊ − ω₋)/2."""
    s, ct, D, Q, dirs = cx.s, cx.ct, cx.D, cx.Q, cx.dirs
    L.append(f'  const {ct} rho = ' + ' + '.join(f'f{i}' for i in range(Q)) + ';')
    for a in range(D):
        pos = [f'f{i}' for i in range(Q) if dirs[i][a] == 1]
        neg = [f'f{i}' for i in range(Q) if dirs[i][a] == -1]
        L.append(f'  const {ct} m{a} = (' + ' + '.join(pos) + ') - (' + ' + '.join(neg) + ');')
    if s.compressible:
        L.append(f'  const {ct} irho = ({ct})1 / rho;')
    for a in range(D):
        half = f'({ct})0.5 * F{a}' if s.ff else c_(cx, cx.F[a] / 2) if s.fm == 'guo' else None
        m = f'(m{a} + {half})' if s.fm == 'guo' else f'm{a}'      # Guo: velocity shifted by F/2
        L.append(f'  const {ct} u{a} = {m}' + (' * irho;' if s.compressible else ';'))
    L.append(f'  const {ct} usq = ' + ' + '.join(f'u{a} * u{a}' for a in range(D)) + ';')
    smagorinsky_moments(cx, L)
    if s.fm == 'guo':
        L.append(f'  const {ct} uF = ' + ' + '.join(f'u{a} * {Fa(cx, a)}' for a in range(D)) + ';')
        L.append(f'  const {ct} kg = ({ct})1 - ({ct})0.5 * omega;')
    if s.trt is not None:
        if s.trt[0] == 'magic':
            lam = c_(cx, s.trt[1])
            wo = f'(({ct})4 - ({ct})2 * omega) / (({ct})4 * {lam} * omega + ({ct})2 - omega)'
        else:
            wo = c_(cx, s.trt[1])
        L.append(f'  const {ct} w_odd = {wo};')
        L.append(f'  const {ct} ta = ({ct})0.5 * (omega + w_odd), tb = ({ct})0.5 * (omega - w_odd);')


def obstacle_copy(cx, L, p, off, sp, soff, more=()):
    """An obstacle cell keeps its state (forward: ``dst = src``; adjoint: ``out = g``): array ``sp`` at ``soff`` to
    array ``p`` at ``off`` (half floats: the bits themselves, no conversion on the way). ``more``: further lines of
    the branch."""
    A = cx.A
    L.append(f'  const unsigned msk = nbmask[{cx.cell}];')
    L.append(f'  if ((msk >> {SELF_BIT}) & 1u) {{')
    for i in range(cx.Q):
        L.append('    ' + (A.copy(p, i, off, sp, soff) if cx.s.h else A.store(p, i, off, A.load(sp, i, soff))))
    L.extend(more)
    L.append('    return;\n  }')


def forward_cell(cx, L):
    """``lbm_fwd_cell``: pull (with the walls' links), collide, store.

    SRT: ``dst_i = f_i + ω (feq_i − f_i)``. TRT, with a = (ω₊ + ω₋)/2, b = (ω₊ − ω₋)/2: ``dst_i = (1 − a) f_i −
    b f_ī + a feq_i + b feq_ī``. MRT: ``dst = f − A (f − feq)``, ``A = ω P_ω + C``.
    Force: 'simple' adds the constant 3 w_i (c_i·F) to every fluid cell's post-collision value; 'guo' shifts the
    velocity by F/2 (/ρ) and adds w_i (1 − ω/2)(3 (c_i − u)·F + 9 (c_i·u)(c_i·F))."""
    s, A, ct, Q, w = cx.s, cx.A, cx.ct, cx.Q, cx.w
    L.append(f'{cx.fn} void lbm_fwd_cell({cx.sig["fwd"]}, const int z, const int y, const int x)\n{{')
    L.append(f'  (void)Z; (void)s_bytes; (void)d_bytes; (void)wallid; {cx.fstr_unused}')
    A.resource(L, 's')
    A.resource(L, 'd')
    wrap_lines(L, cx.axes)
    A.neighbour_offsets(L, 's')
    dcoff = A.cell_offset(L, 'd')
    macroscopic.cell_offsets(cx, L)
    if s.walls:
        obstacle_copy(cx, L, 'd', dcoff, 's', f'so_{cx.centre}', macroscopic.obstacle_zero(cx))

    force_loads(cx, L)
    omega_load(cx, L)
    solid_load(cx, L)
    cell_density(cx, L)
    pull_loads(cx, L)
    moments(cx, L)
    if s.trt is not None or s.mrt is not None:
        # TRT / MRT: every population's equilibrium first (the collision of i reads feq of other populations too)
        for i in range(Q):
            L.append(f'  {ct} fe{i};')
            cu_poly(cx, L, i)
            L.append(f'    fe{i} = {feq(cx, i)}; }}')
        if s.mrt is not None:
            L.append(f'  const {ct} ' + ', '.join(f'nq{k} = f{k} - fe{k}' for k in range(Q)) + ';')   # f − feq
    macroscopic.forward_sums(cx, L)
    for i in range(Q):
        cu_poly(cx, L, i)
        term = ''
        if s.fm == 'simple' and cFi(cx, i):
            term = f' + {c_(cx, 3 * w[i])} * {cFi(cx, i)}' if s.ff else f' + {c_(cx, 3 * w[i] * cx.cF[i])}'
        elif s.fm == 'guo':
            term = (f' + {c_(cx, w[i])} * kg * (({ct})3 * ({cFi(cx, i) or c_(cx, 0)} - uF)'
                    + (f' + {cFi(cx, i, 9)} * cu' if cFi(cx, i) else '') + ')')
        if s.trt is not None:
            j = cx.inv[i]
            val = (f'(({ct})1 - ta) * f{i} - tb * f{j} + ta * fe{i} + tb * fe{j}{term}' if j != i else
                   f'f{i} + omega * (fe{i} - f{i}){term}')
        elif s.mrt is not None:
            pw, cc = mat_row(cx, s.mrt[0], 'nq', i), mat_row(cx, s.mrt[1], 'nq', i)
            val = f'f{i}' + (f' - omega * ({pw})' if pw else '') + (f' - ({cc})' if cc else '') + term
        else:
            val = f'f{i} + omega * ({feq(cx, i)} - f{i}){term}'
        val = macroscopic.forward_value(cx, L, i, forward_blend(cx, i, val) + shift(cx, i, ' - '))
        L.append('    ' + A.store('d', i, dcoff, val) + ' }')
    macroscopic.forward_store(cx, L)
    L.append('}')
