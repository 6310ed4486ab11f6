"""The per-cell solid fraction (``solid_field``, partial bounce-back): its load, the forward blend, the adjoint blend
and the adjoint ``dσ``.

Forward, with ``f_i`` the pulled pdfs (the walls' links applied, zero-centred storage with ``w_i`` added back) and
``c_i`` the collision's value with its force term: ``dst_i = (1 − σ) c_i + σ f_ī``. The adjoint is linear in ``g``, so
the blend is applied to the finished plain values: ``v_j = (1 − σ) v_j^plain + σ g_ĵ``, the field adjoints ``dω`` /
``dF`` are scaled by ``1 − σ``, and

    dσ = Σ_i g_i (f_ī − c_i),    c = f − K (f − feq) + term,   h = Kᵀ g  (SRT ω g; TRT a g_i + b g_ī; MRT Aᵀ g)
       = Σ_k (h_k + g_k̄ − g_k) f_k              (``solid_adjoint_pdfs``: right after the moments; Σ_i g_i f_ī = Σ_k g_k̄ f_k)
         − Σ_k h_k feq_k − Σ_i g_i term_i       (``solid_adjoint``: the equilibria recomputed from ρ, u)

— no second collision pass, and no ``f_k`` held in a register through the adjoint's sums. ``omega`` is the rate the
collision read (Smagorinsky: the effective one; its chain is part of ``v^plain`` and of ``dω``, not of ``dσ``)."""
from .common import c_, cFi, cu_poly, feq, mat_row


def solid_load(cx, L):
    """The cell's solid fraction ``sfr`` and ``sfr1 = 1 − σ`` (``solid_field``)."""
    if not cx.s.sf:
        return
    L.append('  const IDX pc = ' + ' + '.join(f'(IDX){a} * p_{a}' for a in cx.axes) + ';')
    L.append(f'  const {cx.ct} sfr = ({cx.ct})sigf[pc], sfr1 = ({cx.ct})1 - sfr;')


def forward_blend(cx, i, val):
    """``(1 − σ) c_i + σ f_ī`` around the collision's value ``val`` of direction i (before the zero-centred shift and the
    macroscopic sums: the outputs are those of the stored state)."""
    return f'sfr1 * ({val}) + sfr * f{cx.inv[i]}' if cx.s.sf else val


def adjoint_blend(cx, j, v):
    """``(1 − σ) v_j^plain + σ g_ĵ`` around the plain ``v_j``: everything downstream of ``v`` (the links' γ, ``Rr``, the
    programs' ``G_q``, the fix-up launch's atomic adds) takes the blended value."""
    return f'sfr1 * ({v}) + sfr * g{cx.inv[j]}' if cx.s.sf else v


def field_scale(cx, val):
    """A field adjoint of the collision (``dω``, ``dF``; Smagorinsky's chain included) scaled by ``1 − σ``."""
    return f'sfr1 * ({val})' if cx.s.sf else val


def mrt_h(cx, L):
    """MRT: ``h = Aᵀ g`` (``adjoint.adjoint_sums`` prints it where there is no solid fraction)."""
    s = cx.s
    for i in range(cx.Q):
        pw, cc = mat_row(cx, s.mrt[0], 'g', i, True), mat_row(cx, s.mrt[1], 'g', i, True)
        hv = ' + '.join(t for t in ((f'omega * ({pw})' if pw else None), (f'({cc})' if cc else None)) if t)
        L.append(f'  const {cx.ct} h{i} = {hv or c_(cx, 0)};')


def _h(cx, k):
    """``h_k = (Kᵀ g)_k`` as an expression."""
    s = cx.s
    if s.mrt is not None:
        return f'h{k}'
    if s.trt is not None and cx.inv[k] != k:
        return f'(ta * g{k} + tb * g{cx.inv[k]})'
    return f'omega * g{k}'


def solid_adjoint_pdfs(cx, L):
    """``solid_field``: the part of ``dσ`` that reads the pulled pdfs, ``dsf = Σ_k (h_k + g_k̄ − g_k) f_k`` (one pdf per
    term, as ``omega_adjoint_pdfs``) — taken right after the moments (MRT: ``h`` is formed here, ahead of the sums that
    read it)."""
    s = cx.s
    if not s.sf:
        return
    if s.mrt is not None:
        mrt_h(cx, L)
    L.append(f'  {cx.ct} dsf = 0;')
    for i in range(cx.Q):
        j = cx.inv[i]
        L.append(f'  dsf += ({_h(cx, i)}' + (f' + g{j} - g{i}' if j != i else '') + f') * f{i};')


def solid_adjoint(cx, L):
    """``solid_field``: ``dsf −= Σ_k h_k feq_k + Σ_i g_i term_i`` and the cell's ``dσ(x)`` ACCUMULATED into ``dsolid``
    (the strides of the σ field; every fluid cell by one thread of one adjoint launch per step — a listed cell by the
    fix-up launch — so the T steps sum into one zeroed array without atomics; obstacle cells add nothing)."""
    s, ct, w = cx.s, cx.ct, cx.w
    if not s.sf:
        return
    for i in range(cx.Q):
        cu_poly(cx, L, i)
        L.append(f'    dsf -= {_h(cx, i)} * ({feq(cx, i)});')
        if s.fm == 'simple' and cFi(cx, i):
            term = f'{c_(cx, 3 * w[i])} * {cFi(cx, i)}' if s.ff else c_(cx, 3 * w[i] * cx.cF[i])
            L.append(f'    dsf -= g{i} * {term};')
        elif s.fm == 'guo':
            L.append(f'    dsf -= g{i} * {c_(cx, w[i])} * kg * (({ct})3 * ({cFi(cx, i) or c_(cx, 0)} - uF)'
                     + (f' + {cFi(cx, i, 9)} * cu' if cFi(cx, i) else '') + ');')
        L.append('  }')
    L.append('  dsolid[pc] += (T)dsf;')
