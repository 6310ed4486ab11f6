"""The per-cell relaxation rate (``omega_field``): its load and the adjoint ``dω`` (Smagorinsky's chain starts from it)."""
from .common import c_, cFi, cu_poly, feq, mat_row
from .solid import field_scale


def omega_load(cx, L):
    """The cell's relaxation rate (``omega_field``): every use of ``omega`` after it — the collision, the TRT
    rates, Guo's 1 − ω/2, MRT's ω P_ω — reads this local."""
    if not cx.s.of:
        return
    L.append('  const IDX wc = ' + ' + '.join(f'(IDX){a} * w_{a}' for a in cx.axes) + ';')
    L.append(f'  const {cx.ct} {cx.om0} = ({cx.ct})omf[wc];')


def omega_weight(cx, k):
    """``q_k`` of ``dω = −Σ_k q_k n_k`` (``omega_adjoint``; None where it is the constant 0)."""
    s = cx.s
    if s.trt is not None and cx.inv[k] != k:
        return f'(tap * g{k} + tbp * g{cx.inv[k]})'
    if s.mrt is not None:
        pw = mat_row(cx, s.mrt[0], 'g', k, True)
        return f'({pw})' if pw else None
    return f'g{k}'


def omega_adjoint_pdfs(cx, L):
    """``omega_field``: the part of ``dω`` that reads the pulled pdfs, ``dom = −Σ_k q_k f_k`` — taken right after
    the moments, so that no ``f_k`` stays live through the adjoint's sums (``omega_adjoint`` has the formulas)."""
    s, ct = cx.s, cx.ct
    if not s.of and s.sm is None:
        return
    if s.trt is not None:
        if s.trt[0] == 'magic':
            lam = c_(cx, s.trt[1])
            L.append(f'  const {ct} wden = ({ct})4 * {lam} * omega + ({ct})2 - omega;')
            L.append(f'  const {ct} wodp = -({ct})16 * {lam} / (wden * wden);')
        else:
            L.append(f'  const {ct} wodp = 0;')
        L.append(f'  const {ct} tap = ({ct})0.5 * (({ct})1 + wodp), tbp = ({ct})0.5 * (({ct})1 - wodp);')
    L.append(f'  {ct} dom = 0;')
    for k in range(cx.Q):
        if omega_weight(cx, k):
            L.append(f'  dom -= {omega_weight(cx, k)} * f{k};')


def omega_adjoint(cx, L):
    """``omega_field``: the cell's ``dω(x) = Σ_i g_i ∂dst_i/∂ω``, ACCUMULATED into ``domega`` (the strides of the ω
    field; every cell by one thread of one adjoint launch per step — a listed cell by the fix-up launch, which
    the main launch's prologue left it to — so the T steps sum into one zeroed array without atomics).
    With ``n = f − feq``: ``dω = −Σ_k q_k n_k = −Σ_k q_k f_k`` (``omega_adjoint_pdfs``) ``+ Σ_k q_k feq_k`` (here:
    the equilibria recomputed from ρ, u — no load, and no pdf held in a register for it), a cancelling sum.

    SRT ``q = g``: ``dω = −Σ_i g_i n_i``. TRT ``dst_i = f_i − a n_i − b n_ī``: ``q_k = a′ g_k + b′ g_k̄``, ``a′ =
    (1 + ω₋′)/2``, ``b′ = (1 − ω₋′)/2``, ``ω₋′ = −16Λ / (4Λω + 2 − ω)²`` (magic number) or 0 (a constant odd rate);
    the rest population ``q_0 = g_0``. MRT ``dst = f − (ω P_ω + C) n``: ``q = P_ωᵀ g``. Guo's term
    ``w_i (1 − ω/2) T_i``, ``T_i = 3 (c_i − u)·F + 9 (c_i·u)(c_i·F)``, adds ``−½ Σ_i g_i w_i T_i``."""
    s = cx.s
    if not s.of or s.sm is not None:
        return                                  # (Smagorinsky: ``smagorinsky_adjoint`` has stored it already)
    omega_adjoint_equilibria(cx, L)
    L.append('  domega[wc] += (T)' + (f'({field_scale(cx, "dom")})' if s.sf else 'dom') + ';')


def omega_adjoint_equilibria(cx, L):
    """``dom += Σ_k q_k feq_k`` and Guo's ``−½ Σ_i g_i w_i T_i`` (``omega_adjoint``)."""
    s, ct, w = cx.s, cx.ct, cx.w
    if s.fm == 'guo':
        L.append(f'  {ct} domF = 0;')                 # Σ_i g_i w_i T_i
    for i in range(cx.Q):
        cu_poly(cx, L, i)
        if omega_weight(cx, i):
            L.append(f'    dom += {omega_weight(cx, i)} * ({feq(cx, i)});')
        if s.fm == 'guo':
            L.append(f'    domF += g{i} * {c_(cx, w[i])} * (({ct})3 * ({cFi(cx, i) or c_(cx, 0)} - uF)'
                     + (f' + {cFi(cx, i, 9)} * cu' if cFi(cx, i) else '') + ');')
        L.append('  }')
    if s.fm == 'guo':
        L.append(f'  dom -= ({ct})0.5 * domF;')
