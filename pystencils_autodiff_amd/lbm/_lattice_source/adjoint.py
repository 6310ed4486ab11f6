"""The adjoint cell in scatter form: prologue, moment-like sums, the force adjoint, the scatter and its stores."""
from . import macroscopic
from .addressing import wrap_lines
from .collision import force_loads, moments, obstacle_copy
from .common import Fa, axis_sums, c_, cFi, cu_poly, key, ncell, signed_sum
from .links import (cell_density, fix_loads, program_cases, pull_loads, rho_slot, scatter_programs_fix,
                    scatter_programs_inline)
from .omega import omega_adjoint, omega_adjoint_pdfs, omega_load
from .smagorinsky import sm_fold, sm_P, smagorinsky_adjoint
from .solid import adjoint_blend, field_scale, mrt_h, solid_adjoint, solid_adjoint_pdfs, solid_load
from .spec import FIX_BIT


def adjoint_cell(cx, L):
    """``lbm_adj_cell``: ``v_j = Σ_i g_i ∂dst_i/∂f_j`` of the cell's pulled pdfs through the collision's structure,
    each stored to where the forward pulled ``f_j`` from."""
    s, A, ct = cx.s, cx.A, cx.ct
    L.append(f'{cx.fn} void lbm_adj_cell({cx.sig["adj"]}, const int z, const int y, const int x)\n{{')
    L.append(f'  (void)Z; (void)s_bytes; (void)g_bytes; (void)o_bytes; (void)wallid; {cx.fstr_unused}')
    for p in 'sgo':
        A.resource(L, p)
    wrap_lines(L, cx.axes)
    A.neighbour_offsets(L, 's')
    A.neighbour_offsets(L, 'o')
    gcoff = A.cell_offset(L, 'g')
    if s.walls:
        prologue(cx, L, gcoff)
    macroscopic.cell_offsets(cx, L)
    macroscopic.adjoint_seeds(cx, L)
    for i in range(cx.Q):
        L.append(f'  const {ct} g{i} = {A.load("g", i, gcoff)}{macroscopic.seed(cx, i)};')
    force_loads(cx, L)
    omega_load(cx, L)
    solid_load(cx, L)
    cell_density(cx, L)
    listed = s.fix and bool(s.gq_all)
    if listed:
        fix_loads(cx, L)
    pull_loads(cx, L, cx.adj_progs, hoisted=listed and s.walls)
    moments(cx, L)
    omega_adjoint_pdfs(cx, L)
    solid_adjoint_pdfs(cx, L)
    smagorinsky_adjoint(cx, L)
    if s.rho_links:
        L.append(f'  {ct} Rr = 0;')             # Σ_j βρ_j v_j over the cell's density-weighted links
    gown = s.g_own if s.fix else []
    if gown:
        L.append(f'  {ct} ' + ', '.join(f'G{q} = 0' for q in gown) + ';')      # Σ_j J_jq v_j (link programs)
    adjoint_sums(cx, L)
    force_adjoint(cx, L)
    omega_adjoint(cx, L)
    solid_adjoint(cx, L)
    if s.compressible:
        L.append(f'  const {ct} Bu = ' + ' + '.join(f'B{a} * u{a}' for a in range(cx.D)) + ';')
    for j in range(cx.Q):
        scatter(cx, L, j)
    if s.rho_links:
        # the density term: slot Q of the scratch array with inline link programs, its only slot without
        L.append(f'  if (msk & {cx.low}) rho_adj[{rho_slot(cx)}{cx.cell}] = Rr;')
    if gown:
        # out_q(x) += G_q: after the main launch's store of that entry, or (zeroed entry) in either order with this
        # launch's own atomic store into it — two addends onto zero, so the sum is the same either way
        L.append('  ' + ' '.join(A.atomic_add(A.lane('o', q, cx.centre), f'G{q}') for q in gown))
    L.append('}')


def prologue(cx, L, gcoff):
    """Obstacle cells pass ``g`` through; in the main HIP launch the listed cells only zero entries.

    NEIGHBOUR LINKS AND THE TWO HIP LAUNCHES. The fix-up launch (``scatter_programs_fix``, ``scatter_store``) adds
    atomically — G_k, a neighbour link's J·v, and the regular scatter's adds — and every such add lands on an entry
    (listed cell, component in ``gq_all``): call these the E entries. Listed cells (``fix_cells``, ``FIX_BIT``) are
    the fluid cells next to a program wall AND every fluid cell a neighbour link of those can read; ``gq_all``
    holds every component k a Jacobian entry names (at the cell or at an offset) and every direction d with a
    neighbour link.
    The main launch never adds atomically. Its thread of a listed cell y only zeroes, here: E entry (y, q) is
    zeroed iff its regular writer runs in the fix-up launch (y + c_q a wall: y itself, bounced; or y + c_q listed);
    otherwise the writer is an unlisted fluid cell, which stores the entry in the main launch and nobody zeroes it.
    One plain write per E entry in the main launch, then. An entry out_k(x) that receives G_k and whose writer
    x + c_k (or x itself, bounced) is a listed cell too gets the writer's value and G_k by atomic adds — two addends
    onto zero, the same sum in either order, so the result is the one a second fix-up launch (``out += G`` after
    every other store) would give."""
    s, A = cx.s, cx.A
    obstacle_copy(cx, L, 'o', f'oo_{cx.centre}', 'g', gcoff)
    if s.mode != 'main':
        return
    # a cell next to a program wall is the fix-up kernel's: it only zeroes the entries out_q(x), q in gq, that
    # the fix-up kernel adds its G_q into and whose writer also runs there (the cell itself when x + c_q is a
    # wall, or a listed neighbour x + c_q) — both contributions then arrive by atomic adds onto that zero
    L.append(f'  if ((msk >> {FIX_BIT}) & 1u) {{')
    for q in s.gq_all:
        zero = A.store('o', q, f'oo_{cx.centre}', c_(cx, 0))
        if any(cx.dirs[q]):
            iq = cx.inv[q]
            kn = key(cx, iq)                       # the neighbour x + c_q = x - c_(inv q)
            L.append(f'    if (((msk >> {iq}) & 1u) || ((nbmask[{ncell(cx, kn)}] >> {FIX_BIT}) & 1u)) {zero}')
        else:
            L.append(f'    {zero}')
    L.append('    return;\n  }')


def adjoint_sums(cx, L):
    """The moment-like sums of the adjoint in scatter form (``_method.create_lb_adjoint_rule``):
    ``v_j = (1 − ω) g_j + ω (A + Σ_a B_a ∂u_a/∂f_j)`` with S = Σ_i g_i w_i, A = Σ_i g_i w_i (1 + poly_i) and
    B_a = Σ_i g_i w_i (3 + 9 c_i·u) c_ia (− 3 u_a S, in ``force_adjoint``).
    TRT takes them over h_i = a g_i + b g_ī: ``v_j = (1 − a) g_j − b g_ĵ + A_h + Σ_a B_h,a ∂u_a/∂f_j``; MRT over
    h = Aᵀ g: ``v_j = g_j − h_j + A_h + Σ_a B_h,a ∂u_a/∂f_j``."""
    s, ct, D, w = cx.s, cx.ct, cx.D, cx.w
    if s.mrt is not None and not s.sf:
        # h = Aᵀ g (with a solid fraction ``solid_adjoint_pdfs`` has formed it already)
        mrt_h(cx, L)
    L.append(f'  {ct} S = 0, A = 0;')
    if s.gsplit:
        L.append(f'  {ct} Sg = 0;')                   # Σ_i g_i w_i (the force term's sums run over g)
    for a in range(D):
        L.append(f'  {ct} B{a} = 0;')
        if s.gsplit:
            L.append(f'  {ct} Bg{a} = 0;')            # Σ_i g_i w_i (3 + 9 c_i·u) c_ia
        if s.fm == 'guo':
            L.append(f'  {ct} E{a} = 0;')           # Σ_i g_i w_i c_ia (c_i·F)
        if s.ff and s.fm == 'simple':
            L.append(f'  {ct} M{a} = 0;')           # Σ_i g_i w_i c_ia (the 'simple' force adjoint / 3)
    for i in range(cx.Q):
        cu_poly(cx, L, i, poly=False)
        if s.trt is not None:
            # the equilibrium sums over h_i = a g_i + b g_ī (rest population: ω g_0)
            hi = f'(ta * g{i} + tb * g{cx.inv[i]})' if cx.inv[i] != i else f'omega * g{i}'
        else:
            # (Smagorinsky, SRT: h_i = ω g_i — the scatter then has no ω in front of the equilibrium part)
            hi = f'h{i}' if s.mrt is not None else f'omega * g{i}' if s.sm is not None else f'g{i}'
        hi = sm_fold(cx, i, hi)
        L.append(f'    const {ct} gw = {hi} * {c_(cx, w[i])};')
        L.append('    S += gw;')
        if s.gsplit:
            L.append(f'    const {ct} gwg = g{i} * {c_(cx, w[i])};')
            L.append('    Sg += gwg;')
        if s.compressible:
            L.append(f'    A += gw * (({ct})1 + cu * (({ct})3 + ({ct})4.5 * cu) - ({ct})1.5 * usq);')
        if any(cx.dirs[i]):
            L.append(f'    const {ct} t = gw * (({ct})3 + ({ct})9 * cu);')
            axis_sums(cx, L, i, 'B', 't')
            if s.gsplit:
                L.append(f'    const {ct} tg = gwg * (({ct})3 + ({ct})9 * cu);')
                axis_sums(cx, L, i, 'Bg', 'tg')
            if s.fm == 'guo' and cFi(cx, i):
                L.append(f'    const {ct} tf = {"gwg" if s.gsplit else "gw"} * {cFi(cx, i)};')
                axis_sums(cx, L, i, 'E', 'tf')
            if s.ff and s.fm == 'simple':
                axis_sums(cx, L, i, 'M', f'(g{i} * {c_(cx, w[i])})' if s.trt is not None or s.mrt is not None
                          else 'gw')
        L.append('  }')
    if not s.compressible:
        L.append('  A = S;')


def force_adjoint(cx, L):
    """The velocity sensitivities B_a finished, with the force's part in them, and the force field's adjoint.

    'simple' leaves the adjoint unchanged. 'guo': the force term's derivative through u joins the velocity
    sensitivities: B_a += C_a / ω with C_a = (1 − ω/2) Σ_i g_i w_i (9 c_ia (c_i·F) − 3 F_a).
    ``force_field``: the adjoint ACCUMULATES the force adjoint into ``dforce`` (the strides of ``force``; every cell
    by one thread, so the T steps of the time-step op sum into one zeroed array): 'simple' ``dF_a = 3 Σ_i g_i w_i
    c_ia``; 'guo' — through the explicit term and the velocity shift ``∂u_a/∂F_a = 1/2 (/ρ)`` — ``dF_a = (1 − ω/2)
    Bf_a + ω B_a / 2 (/ρ)`` with ``Bf_a`` the equilibrium part of the velocity sensitivity (before the ρ scaling)
    and ``B_a`` the full one."""
    s, ct = cx.s, cx.ct
    for a in range(cx.D):
        L.append(f'  B{a} -= ({ct})3 * u{a} * S;')
        if s.ff and s.fm == 'guo':
            # the explicit force term's F-derivative sums (over g: Bg for TRT / MRT, = B before the ρ scaling for
            # SRT)
            L.append(f'  const {ct} Bf{a} = ' + (f'Bg{a} - ({ct})3 * u{a} * Sg;' if s.gsplit else f'B{a};'))
        if s.compressible:
            L.append(f'  B{a} *= rho;')
        if s.gsplit:
            # the force term's derivative through u (TRT / MRT: v = g − h + A_h + Σ B_a ∂u_a/∂f_j, no ω factor)
            L.append(f'  B{a} += kg * (({ct})9 * E{a} - ({ct})3 * {Fa(cx, a)} * Sg);')
        elif s.fm == 'guo':
            # the force term's derivative through u, scaled into B (v = … + ω (A + Σ B_a ∂u_a/∂f_j))
            L.append(f'  B{a} += kg * (({ct})9 * E{a} - ({ct})3 * {Fa(cx, a)} * S) / omega;')
    if not s.ff:
        return
    # the force adjoint of this cell, accumulated over the op's steps
    for a in range(cx.D):
        if s.fm == 'simple':
            val = f'({ct})3 * M{a}'
        else:
            # through the explicit term, and through the velocity shift ∂u_a/∂F_a = 1/2 (/ρ): Σ_i g_i ∂dst_i/∂u_a,
            # which is ω B_a for SRT (B carries 1/ω) and B_a for TRT / MRT
            sc = '' if s.gsplit else 'omega * '
            val = f'kg * Bf{a} + ({ct})0.5 * {sc}B{a}' + (' * irho' if s.compressible else '')
        L.append(f'  dforce[(IDX){a} * f_c + fc] += {field_scale(cx, val)}{macroscopic.force_seed(cx, a)};')


def scatter(cx, L, j):
    """``v_j``, stored to the cell the forward pulled ``f_j`` from — ``(x − c_j, j)``, or ``(x, ī)`` for a bounced
    ``f_j`` (scaled by the link's γ). Without link programs every (component, cell) of the result is written
    exactly once (for fluid ``x``: by ``x + c_k`` if that cell is fluid, else by ``x`` itself; obstacle cells by
    themselves), so the output needs no zero fill and no atomics."""
    s, ct, Q, inv = cx.s, cx.ct, cx.Q, cx.inv
    cbs = signed_sum(cx, j, 'B', paren=False) or f'({ct})0'
    du = f'(({cbs}) - Bu) * irho' if s.compressible else f'({cbs})'
    linked = s.walls and any(cx.dirs[j]) and s.links is not None
    vq = '' if linked else 'const '
    # Smagorinsky: + dom ∂ω_eff/∂f_j beside the folded sums (``smagorinsky_adjoint``)
    sm = '' if s.sm is None else (f' + sm_l * {sm_P(cx, j)}' if sm_P(cx, j) else '') + \
        (' - sm_c' if s.compressible else '')
    if s.trt is not None and inv[j] != j:
        v = f'(({ct})1 - ta) * g{j} - tb * g{inv[j]} + (A + {du}){sm}'
    elif s.trt is not None:
        v = f'(({ct})1 - omega) * g{j} + (A + {du}){sm}'
    elif s.mrt is not None:
        v = f'g{j} - h{j} + (A + {du}){sm}'
    elif s.sm is not None:
        v = f'(({ct})1 - omega) * g{j} + (A + {du}){sm}'
    else:
        v = f'(({ct})1 - omega) * g{j} + omega * (A + {du})'
    L.append(f'  {{ {vq}{ct} v = {adjoint_blend(cx, j, v)};')
    taken = ''                  # (fix-up kernel) guard of the scatter store: not where a neighbour link is taken
    if linked:
        if s.rho_links:
            L.append(f'    if ((msk >> {j}) & 1u) Rr += lk_gr[id{j} * {Q} + {j}] * v;')
        cases = program_cases(cx, j) if cx.adj_progs else []
        if cases:
            taken = (scatter_programs_fix if s.fix else scatter_programs_inline)(cx, L, j, cases)
        L.append(f'    if ((msk >> {j}) & 1u) v *= lk_g[id{j} * {Q} + {j}];')
    scatter_store(cx, L, j, taken)


def scatter_store(cx, L, j, taken):
    """The store of ``v_j`` (closes the component's block), in three flavours: a plain store; one store whose
    per-lane offset selects the bounced or the pulled-from entry (walls); or, in the fix-up launch, that store as
    an atomic add where its target is an E entry (``prologue``):
    in the fix-up launch every scatter store whose target is an E entry is an atomic add (bounced: the cell itself
    is listed, atomic iff ī_j in ``gq_all``; to x − c_j: atomic iff j in ``gq_all`` and that cell has ``FIX_BIT``);
    its remaining plain stores go to entries that are not E, which receive no add at all.
    Hence no entry is written by a plain store in the launch that atomically adds into it; the stores of the main
    launch come first in stream order; and an E entry whose regular writer is in the fix-up launch starts from zero
    and receives that writer's value as one of the adds. A taken neighbour link's entry (x, d) has no regular writer
    left: it is d in ``gq_all`` that gets it zeroed (x + c_d is a wall), and other links may add into it.
    Bitwise reproducibility: own-cell programs and flat neighbour-link walls put at most two nonzero addends on an
    entry (one order-independent sum); neighbour links can put three or more on one (corners, a cell read by
    several links) — there, and only there, the result may differ in the last bit from run to run. Lattices
    without neighbour links get the source they always had, to the byte."""
    s, A, inv = cx.s, cx.A, cx.inv
    k = key(cx, j)
    gq = s.gq_all if s.fix else []
    walled = s.walls and any(cx.dirs[j])
    bounced, pulled = A.lane('o', inv[j], cx.centre), A.lane('o', j, k)
    if walled and (j in gq or inv[j] in gq):
        # a store into a G entry (component q in gq of a listed cell) is an atomic add onto the entry the main
        # kernel zeroed: the cell itself (bounced, component ī) or a listed neighbour x − c_j (component j)
        ab = 'true' if inv[j] in gq else 'false'
        an = f'((nbmask[{ncell(cx, k)}] >> {FIX_BIT}) & 1u)' if j in gq else 'false'
        L.append(f'    const {A.off_type} vs = ((msk >> {j}) & 1u) ? {bounced} : {pulled};')
        L.append(f'    {taken}if (((msk >> {j}) & 1u) ? {ab} : {an}) {A.atomic_add("vs", "(T)v")} '
                 f'else {A.store_v("o", "vs", "v")} }}' + (' }' if taken else ''))
    elif walled:
        A.select_store(L, 'o', j, bounced, pulled, 'v')
    elif j in gq:
        # the rest population of a listed cell: its own G entry
        L.append(f'    {A.atomic_add(pulled, "(T)v")} }}')
    else:
        L.append('    ' + A.store('o', j, f'oo_{k}', 'v') + ' }')
