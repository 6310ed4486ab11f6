"""The walls' links: coefficient tables, the pull with its links and programs, the fix-up kernel's loads, the
programs' part of the scatter and the adjoint's second pass."""
import re

from .addressing import cell_offset, wrap_lines
from .common import key, ncell, shift
from .spec import SELF_BIT, _key


def omask(cx, pg):
    """Mask bits of the cells a neighbour link reads (bit ī_o of a cell's mask: x + c_o is a wall — the same
    fact as that cell's own ``SELF_BIT``, without loading its mask word)."""
    return f'{sum(1 << cx.inv[o] for o in pg.reads)}u'


def okey(cx, o):
    return _key(cx.dirs[cx.inv[o]])                    # x + c_o = x − c_ī(o)


def nb_loads(cx, code, rd):
    """Loads of the neighbours' pdfs a program's code reads (``const T n<o>_<k> = src_k(x + c_o);``)."""
    used = sorted({(int(o), int(k)) for o, k in re.findall(r'\bn(\d+)_(\d+)\b', code)})
    return ' '.join(f'const {cx.ct} n{o}_{k} = {rd(k, okey(cx, o))};' for o, k in used)


def own_loads(cx, code, rd):
    """Loads of the cell's own pdfs a program's code reads (``const T c<q> = …;``; ``rd(q)``: the load)."""
    used = sorted({int(m) for m in re.findall(r'\bc(\d+)\b', code)})
    return ' '.join(f'const {cx.ct} c{q} = {rd(q)};' for q in used)


def program_cases(cx, i):
    """(wall id, program of the link pulled as component i: direction ī) for the ids with link programs."""
    if not cx.s.gen or not any(cx.dirs[i]):
        return []
    ii = cx.inv[i]
    return [(wid, wall[ii]) for wid, wall in enumerate(cx.s.progs) if wall is not None and wall[ii] is not None]


def link_tables(cx, L):
    """Per (wall id, pulled component j): the link of direction d = ī_j (the population that left x towards the
    wall cell x + c_d = x − c_j comes back as j)."""
    s, Q = cx.s, cx.Q
    if s.links is None:
        return
    # (half pdfs: the coefficients stay in the compute type)
    qual = ('__constant__ ' if s.hip else 'static const ') + (cx.ct if s.h else 'T')
    cols = (('lk_a', 'alpha'), ('lk_b', 'beta'), ('lk_g', 'gamma')) + \
        ((('lk_r', 'beta_rho'), ('lk_gr', 'gamma_rho')) if s.rho_links else ())
    for nm, col in cols:
        vals = [repr(getattr(lk[cx.inv[j]], col)) for lk in s.link_rows for j in range(Q)]
        L.append(f'{qual} {nm}[{len(vals)}] = {{{", ".join(vals)}}};')


def pull_loads(cx, L, progs=True, hoisted=False):
    """``f_i``: the pulled pdfs of the cell — ``src_i(x − c_i)``, or the link of the wall cell there (bounce-back
    ``src_ī(x)``, its table row ``α f + β (+ βρ ρ)``, or its program).
    ``hoisted`` (the fix-up kernel, whose every cell has program links): the wall ids are loaded for every
    direction up front and the cell's own pdfs ``c<q>`` are already loaded, so no load waits on the mask."""
    s, A, ct, Q, centre = cx.s, cx.A, cx.ct, cx.Q, cx.centre
    for i in range(Q):
        k = key(cx, i)
        if not (s.walls and any(cx.dirs[i])):
            L.append(f'  const {ct} f{i} = {A.load("s", i, f"so_{k}")}{shift(cx, i)};')
            continue
        cq = '' if s.links is not None else 'const '
        bounced, pulled = A.lane('s', cx.inv[i], centre), A.lane('s', i, k)
        if hoisted and A.buf:
            # (fix-up kernel: both candidates loaded, then selected — no load waits on the mask)
            L.append(f'  const {ct} fb{i} = {A.load_v("s", bounced)}, fs{i} = {A.load_v("s", pulled)};')
            L.append(f'  {cq}{ct} f{i} = ((msk >> {i}) & 1u) ? fb{i} : fs{i};')
        else:
            # a bounced component is read from the cell itself
            A.select_load(L, f'{cq}{ct} f{i}', 's', i, bounced, pulled, shift(cx, i))
        if s.links is None:
            continue
        # the wall cell's link (moving wall: α = 1, β = 6 w (c·u)); its id is loaded on this path only
        rterm = f' + lk_r[id{i} * {Q} + {i}] * rs' if s.rho_links else ''
        link = f'f{i} = lk_a[id{i} * {Q} + {i}] * f{i} + lk_b[id{i} * {Q} + {i}]{rterm};'
        if hoisted:
            L.append(f'  const unsigned id{i} = ((msk >> {i}) & 1u) ? (unsigned)wid{i} : 0u;')
            L.append(f'  if ((msk >> {i}) & 1u) {link}')
        else:
            L.append(f'  unsigned id{i} = 0;')
            L.append(f'  if ((msk >> {i}) & 1u) {{ id{i} = wallid[{ncell(cx, k)}]; {link} }}')
        cases = program_cases(cx, i) if progs else []
        if cases:
            L.append(f'  if ((msk >> {i}) & 1u) switch (id{i}) {{')
            for wid, pg in cases:
                body = ' '.join(pg.lines) + f' f{i} = {pg.value};'
                ld = '' if hoisted else own_loads(cx, body, lambda q: A.load('s', q, f'so_{centre}'))
                if pg.neighbour:
                    # a neighbour link: taken where every cell it reads is fluid, else f_i stays the
                    # bounce-back the table row (1, 0) made
                    nl = nb_loads(cx, body, lambda q, kk: A.load('s', q, f'so_{kk}'))
                    L.append(f'    case {wid}: if (!(msk & {omask(cx, pg)})) {{ {ld} {nl} {body} }} break;')
                else:
                    L.append(f'    case {wid}: {{ {ld} {body} }} break;')
            L.append('    default: break;\n  }')


def cell_density(cx, L):
    """ρ(x) of the cell's own (pre-streaming) pdfs, for density-weighted links, on cells next to a wall."""
    if not cx.s.rho_links:
        return
    L.append(f'  {cx.ct} rs = 0;')
    L.append(f'  if (msk & {cx.low}) rs = ' + ' + '.join(cx.A.load('s', q, f'so_{cx.centre}')
                                                       for q in range(cx.Q)) + ';')


def fix_loads(cx, L):
    """The fix-up kernel: every listed cell has a program link, so its own pdfs (read by the links' programs and
    their Jacobians) and the wall ids of all its neighbours are loaded once, up front, beside the mask — no load
    of the kernel's latency-bound chain waits on the mask or on an id."""
    s = cx.s
    used = sorted({int(m) for wall in s.progs if wall is not None for pg in wall if pg is not None
                   for m in re.findall(r'\bc(\d+)\b', ' '.join(pg.lines) + ' ' + pg.value + ' ' +
                                       ' '.join(' '.join(r.lines) + ' ' + r.expr for r in pg.jac))})
    if used:
        L.append('  ' + ' '.join(f'const {cx.ct} c{q} = {cx.A.load("s", q, f"so_{cx.centre}")};'
                                 for q in used))
    if s.walls:
        L.append('  ' + ' '.join(f'const unsigned char wid{i} = wallid[{ncell(cx, key(cx, i))}];'
                                 for i in range(cx.Q) if any(cx.dirs[i])))


def scatter_programs_fix(cx, L, j, cases):
    """(Fix-up kernel) a program-linked component: Σ_j J_jq(c) v_j (c: the cell's own pre-streaming pdfs) into the
    G accumulators. A neighbour link (``LinkProgram.reads``: the offsets it reads; Jacobian entries with an
    ``offset``) may read ``src_k(x + c_o)``. It is taken where every cell ``x + c_o`` it reads is fluid:
    bit ī_o of the cell's OWN mask word says so (it is the neighbour's ``SELF_BIT``, already in a register); it
    is the bounce-back otherwise: the wall id's table row is (α, β, γ) = (1, 0, 1), so the fused path has made
    ``f_j = src_ī(x)`` before the link's ``case`` and scatters ``v_j`` to ``(x, ī_j)`` after it. A taken link
    replaces both: the forward overwrites ``f_j``; the adjoint adds ``J·v_j`` into ``out_k(x + c_o)`` and drops the
    scatter to ``(x, ī_j)`` (the store is skipped: returns its guard)."""
    A = cx.A
    taken = ''
    if any(pg.neighbour for _, pg in cases):
        L.append('    int tk = 0;')
        taken = 'if (!tk) { '
    L.append(f'    if ((msk >> {j}) & 1u) switch (id{j}) {{')
    for wid, pg in cases:
        if pg.neighbour:
            # a neighbour link, where every cell it reads is fluid: J·v into the cells it read (atomic
            # adds: those entries are zeroed or stored by the main launch), and no bounce-back store
            # (``tk``: the zeroed entry of direction ī_j stays as it is)
            rows = ' '.join('{ ' + ' '.join(r.lines) + ' ' +
                            (f'G{r.component} += ({r.expr}) * v;' if r.own else
                             A.atomic_add(A.lane('o', r.component, okey(cx, r.offset)), f'(T)(({r.expr}) * v)')) +
                            ' }' for r in pg.jac)
            nl = nb_loads(cx, rows, lambda q, kk: A.load('s', q, f'so_{kk}'))
            L.append(f'      case {wid}: if (!(msk & {omask(cx, pg)})) {{ {nl} {rows} tk = 1; }} break;')
            continue
        if len({r.lines for r in pg.jac}) == 1:
            # one set of temporaries for the whole row (FixedDensity.program): emitted once
            rows = ' '.join(pg.jac[0].lines) + ' ' + ' '.join(f'G{r.component} += ({r.expr}) * v;' for r in pg.jac)
        else:
            rows = ' '.join('{ ' + ' '.join(r.lines) + f' G{r.component} += ({r.expr}) * v; }}' for r in pg.jac)
        L.append(f'      case {wid}: {{ {rows} }} break;')
    L.append('      default: break;\n    }')
    return taken


def scatter_programs_inline(cx, L, j, cases):
    """(C target) a program-linked component: its v for the second pass (the Jacobian row is evaluated there). The
    first pass writes every entry once, so where a neighbour link is taken it stores a zero to the bounce-back's
    entry ``(x, ī_j)``."""
    slot = f'rho_adj[(IDX){j} * {cx.ncells} + {cx.cell}]'
    L.append(f'    if ((msk >> {j}) & 1u) switch (id{j}) {{')
    own = [wid for wid, pg in cases if not pg.neighbour]
    if own:
        L.append('      ' + ' '.join(f'case {wid}:' for wid in own) + f' {slot} = v; break;')
    for wid, pg in cases:
        if pg.neighbour:
            # a neighbour link where it is taken: v for the second pass, a zero for the bounce-back's entry
            L.append(f'      case {wid}: if (!(msk & {omask(cx, pg)})) {{ {slot} = v; v = 0; }} break;')
    L.append('      default: break;\n    }')
    return ''


def rho_slot(cx):
    return f'(IDX){cx.Q} * {cx.ncells} + ' if cx.s.inl else ''


def rho_cell(cx, L):
    """``lbm_adj_rho_cell``: the density term of the cell's links reaches every component of the cell, whose adjoint
    entries the first pass wrote from other threads; with inline link programs (the C target) also ``Σ_j J_jk(c)
    v_j`` into component k of the cell, and a taken neighbour link's ``J·v`` into ``out_k(x + c_o)`` (``rho_adj``
    holds ``v_j``). That writes OTHER cells from other OpenMP threads: with neighbour links every update of this
    pass is an ``omp atomic`` one."""
    s, ct, Q = cx.s, cx.ct, cx.Q
    L.append(f'{cx.fn} void lbm_adj_rho_cell({cx.sig["adj_rho"]}, const int z, const int y, const int x)\n{{')
    L.append('  (void)Z;')
    L.append(f'  const unsigned msk = nbmask[{cx.cell}];')
    L.append(f'  if (((msk >> {SELF_BIT}) & 1u) || !(msk & {cx.low})) return;')
    L.append(cell_offset('o', cx.axes))
    at = '_Pragma("omp atomic") ' if s.nb and not s.hip else ''
    if s.rho_links:
        L.append(f'  const {ct} R = rho_adj[{rho_slot(cx)}{cx.cell}];')
        for q in range(Q):
            L.append(f'  {at}out[(IDX){q} * o_q + oc] += R;')
    if not s.inl:
        L.append('}')
        return
    # Σ_j J_jk(c) v_j over the cell's program-linked components (c: the cell's own pre-streaming pdfs)
    wrap_lines(L, cx.axes)
    L.append(cell_offset('s', cx.axes))
    if s.nb:
        cx.A.neighbour_offsets(L, 's')
        cx.A.neighbour_offsets(L, 'o')

    def own(q):
        return f'({ct})src[(IDX){q} * s_q + sc]'
    for j in range(Q):
        cases = program_cases(cx, j)
        if not cases:
            continue
        L.append(f'  if ((msk >> {j}) & 1u) {{')
        L.append(f'    const {ct} v = rho_adj[(IDX){j} * {cx.ncells} + {cx.cell}];')
        L.append(f'    switch (wallid[{ncell(cx, key(cx, j))}]) {{')
        for wid, pg in cases:
            if pg.neighbour:
                # a neighbour link, where it is taken: J·v into out_k(x + c_o)
                rows = ' '.join('{ ' + ' '.join(r.lines) + f' {at}out[(IDX){r.component} * o_q + ' +
                                ('oc' if r.own else f'oo_{okey(cx, r.offset)}') + f'] += ({r.expr}) * v; }}'
                                for r in pg.jac)
                nl = nb_loads(cx, rows, lambda q, kk: f'({ct})src[(IDX){q} * s_q + so_{kk}]')
                L.append(f'      case {wid}: if (!(msk & {omask(cx, pg)})) {{ {own_loads(cx, rows, own)} {nl} '
                         f'{rows} }} break;')
                continue
            rows = ' '.join('{ ' + ' '.join(r.lines) + f' {at}out[(IDX){r.component} * o_q + oc] += ({r.expr}) * v; }}'
                            for r in pg.jac)
            L.append(f'      case {wid}: {{ {own_loads(cx, rows, own)} {rows} }} break;')
        L.append('      default: break;\n    }\n  }')
    L.append('}')
