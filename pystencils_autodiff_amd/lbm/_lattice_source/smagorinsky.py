"""The Smagorinsky subgrid model: the effective rate, its moments in the cell and the adjoint's chain factors."""
from .common import c_
from .omega import omega_adjoint_equilibria


def smagorinsky_rate(cx, L):
    """``lbm_omega_eff``, the one definition of the effective rate: ``ω_eff = 2 / (τ0 + R)``, ``τ0 = 1/ω0``,
    ``R = √(τ0² + 18 C_s² q)`` (R is returned too: the adjoint's chain factors read it)."""
    s, ct = cx.s, cx.ct
    if s.sm is None:
        return
    sqrt = '__builtin_sqrt' if ct == 'double' else '__builtin_sqrtf'
    L.append(f'{cx.fn} {ct} lbm_omega_eff(const {ct} omega_0, const {ct} q, {ct}* R)\n{{')
    L.append(f'  const {ct} tau0 = ({ct})1 / omega_0;')
    L.append(f'  *R = {sqrt}(tau0 * tau0 + {c_(cx, 18 * s.sm * s.sm)} * q);')
    L.append(f'  return ({ct})2 / (tau0 + *R);\n}}')


def smagorinsky_moments(cx, L):
    """After ρ, u: ``Π_ab = Σ_i c_ia c_ib (f_i − feq_i)`` with the equilibrium's closed second moments
    ``ρ (δ_ab/3 + u_a u_b)`` (incompressible: ``ρ δ_ab/3 + u_a u_b``; exact for the second-order equilibrium on
    D2Q9, D3Q19 and D3Q27, whose weights are isotropic to fourth order), ``N = √(2 Σ_ab Π_ab²)`` over all D²
    entries, ``q = N/ρ`` (incompressible: ``N``) and ``omega``, the rate everything below reads."""
    s, ct, D = cx.s, cx.ct, cx.D
    if s.sm is None:
        return
    sqrt = '__builtin_sqrt' if ct == 'double' else '__builtin_sqrtf'
    third = c_(cx, 1.0 / 3.0)
    for a in range(D):
        for b in range(a, D):
            pos = [f'f{i}' for i, c in enumerate(cx.dirs) if c[a] * c[b] == 1]
            neg = [f'f{i}' for i, c in enumerate(cx.dirs) if c[a] * c[b] == -1]
            mom = '(' + ' + '.join(pos) + ')' + (' - (' + ' + '.join(neg) + ')' if neg else '')
            uu = f'u{a} * u{b}'
            if a == b:
                eq = f'rho * ({third} + {uu})' if s.compressible else f'(rho * {third} + {uu})'
            else:
                eq = f'rho * {uu}' if s.compressible else uu
            L.append(f'  const {ct} sm_P{a}{b} = {mom} - {eq};')
    diag = ' + '.join(f'sm_P{a}{a} * sm_P{a}{a}' for a in range(D))
    off = ' + '.join(f'sm_P{a}{b} * sm_P{a}{b}' for a in range(D) for b in range(a + 1, D))
    L.append(f'  const {ct} sm_N = {sqrt}(({ct})2 * ({diag}) + ({ct})4 * ({off}));')
    L.append(f'  const {ct} sm_q = sm_N' + (' * irho;' if s.compressible else ';'))
    L.append(f'  {ct} sm_R;')
    L.append(f'  const {ct} omega = lbm_omega_eff({cx.om0}, sm_q, &sm_R);')


def sm_P(cx, i):
    """``P_i = Σ_ab Π_ab c_ia c_ib`` of direction i (None for the rest direction, where it is 0)."""
    c = cx.dirs[i]
    t = [f'sm_P{a}{a}' for a in range(cx.D) if c[a]]
    t += [('- ' if c[a] * c[b] < 0 else '') + f'({cx.ct})2 * sm_P{a}{b}'
          for a in range(cx.D) for b in range(a + 1, cx.D) if c[a] * c[b]]
    return '(' + ' + '.join(t).replace('+ - ', '- ') + ')' if t else None


def smagorinsky_adjoint(cx, L):
    """The chain factors of ``ω_eff(f, ω0)`` once ``dom = Σ_i g_i ∂dst_i/∂ω`` (at ω = ω_eff) is complete:

        v_k += dom ∂ω_eff/∂f_k,   ∂ω_eff/∂f_k = ∂ω_eff/∂q · ∂q/∂f_k,   ∂ω_eff/∂q = −ω_eff² K / (4R),  K = 18 C_s²
        ∂q/∂f_k = (∂N/∂f_k − q)/ρ  (incompressible: ∂N/∂f_k),   ∂N/∂f_k = (2/N)(P_k − Σ_i P_i ∂feq_i/∂f_k)

    With κ = dom ∂ω_eff/∂q and λ = 2κ/(Nρ) (incompressible: 2κ/N): ``v_k += λ P_k − Σ_i λ P_i ∂feq_i/∂f_k − κ q/ρ``
    (the last term compressible only). The middle sum has the form of the equilibrium sums of ``adjoint_sums``:
    they run over ``h_i − λ P_i`` — which is why ``dom`` is finished before them here, not after
    (``omega_adjoint``). Where N = 0, ∂N/∂f_k is defined as 0 (λ = 0): the reciprocal is guarded, no NaN.
    With an ω field: ``domega += dom ∂ω_eff/∂ω0``, ``∂ω_eff/∂ω0 = ω_eff² (1 + τ0/R) / (2 ω0²)``."""
    s, ct = cx.s, cx.ct
    if s.sm is None:
        return
    omega_adjoint_equilibria(cx, L)
    K = c_(cx, 18 * s.sm * s.sm)
    L.append(f'  const {ct} sm_k = -dom * omega * omega * {K} / (({ct})4 * sm_R);')
    L.append(f'  const {ct} sm_iN = sm_N > ({ct})0 ? ({ct})1 / sm_N : ({ct})0;')
    L.append(f'  const {ct} sm_l = ({ct})2 * sm_k * sm_iN' + (' * irho;' if s.compressible else ';'))
    if s.compressible:
        L.append(f'  const {ct} sm_c = sm_k * sm_q * irho;')
    if s.of:
        L.append(f'  domega[wc] += (T)({"sfr1 * " if s.sf else ""}dom * omega * omega * (({ct})1 + (({ct})1 / {cx.om0}) / sm_R) / '
                 f'(({ct})2 * {cx.om0} * {cx.om0}));')


def sm_fold(cx, i, hi):
    """The weight of direction i in the equilibrium sums: ``h_i`` (``hi``), with Smagorinsky ``h_i − λ P_i``."""
    if cx.s.sm is None or not sm_P(cx, i):
        return hi
    return f'({hi} - sm_l * {sm_P(cx, i)})'
