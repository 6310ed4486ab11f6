"""The density and velocity outputs (``macroscopic``): the forward cell writes ρ and u of the state it stores, the
adjoint cell folds their adjoint seeds into ``g`` where it loads it.

Forward, fluid cell: the moments of the post-collision values ``dst_i`` in the compute type, before the cast to the
storage type, as ``_method.macroscopic_getter`` forms them: ρ = Σ_i dst_i (zero-centred: 1 + Σ_i δdst_i), the momentum
Σ_i c_i dst_i (+ F/2 under Guo), divided by ρ for a compressible rule. Obstacle cells get exactly 0.
Adjoint: ``g_i += drho + Σ_a dvel_a ∂u_a/∂dst_i`` with ``∂u_a/∂dst_i = (c_ia − u_a)/ρ`` (compressible: ρ, u are this
step's recorded outputs at the cell) or ``c_ia`` (incompressible: neither is read). Everything after the load takes the
seeded ``g``. Obstacle cells and, in the main HIP launch, the listed cells have returned before (``adjoint.prologue``).
The arrays are of the compute type and read by strides (``r_*``: ρ, ``[*domain]``; ``v_*``: u, ``[*domain, D]``)."""
from .addressing import cell_offset
from .common import axis_sums, c_, signed_sum


def _vel(a):
    return f'(IDX){a} * v_c + vc'


def cell_offsets(cx, L):
    """The cell's offsets ``rc`` / ``vc`` in the ρ and the u arrays."""
    if not cx.s.mo:
        return
    L.append(cell_offset('r', cx.axes))
    L.append(cell_offset('v', cx.axes))
    if cx.D == 2:
        L.append('  (void)r_z; (void)v_z;')


def obstacle_zero(cx):
    """The lines of the forward's obstacle branch."""
    if not cx.s.mo:
        return []
    return ['    rho_out[rc] = 0;'] + [f'    vel_out[{_vel(a)}] = 0;' for a in range(cx.D)]


def forward_sums(cx, L):
    """The accumulators of ρ and the momentum."""
    if cx.s.mo:
        L.append(f'  {cx.ct} mo_r = {1 if cx.s.zc else 0}' + ''.join(f', mo_j{a} = 0' for a in range(cx.D)) + ';')


def forward_value(cx, L, i, val):
    """The stored value of direction i (inside its block): summed into the moments; returns what the store takes."""
    if not cx.s.mo:
        return val
    L.append(f'    const {cx.ct} dv = {val};')
    L.append('    mo_r += dv;')
    axis_sums(cx, L, i, 'mo_j', 'dv')
    return 'dv'


def forward_store(cx, L):
    """ρ and u of the stored state, D + 1 stores."""
    s, ct = cx.s, cx.ct
    if not s.mo:
        return
    if s.compressible:
        L.append(f'  const {ct} mo_ir = ({ct})1 / mo_r;')
    L.append('  rho_out[rc] = mo_r;')
    for a in range(cx.D):
        half = f' + ({ct})0.5 * F{a}' if s.ff else f' + {c_(cx, cx.F[a] / 2)}' if s.fm == 'guo' else ''
        m = f'(mo_j{a}{half})' if s.fm == 'guo' else f'mo_j{a}'
        L.append(f'  vel_out[{_vel(a)}] = {m}' + (' * mo_ir;' if s.compressible else ';'))


def adjoint_seeds(cx, L):
    """``mo_s`` and ``mo_d{a}`` with ``seed_i = mo_s + c_i · mo_d``: incompressible ``drho`` and ``dvel_a``;
    compressible ``drho − Σ_a dvel_a u_a / ρ`` and ``dvel_a / ρ``."""
    s, ct = cx.s, cx.ct
    if not s.mo:
        return
    if s.compressible:
        L.append(f'  const {ct} mo_ir = ({ct})1 / rho_out[rc];')
    for a in range(cx.D):
        L.append(f'  const {ct} mo_d{a} = dvel[{_vel(a)}]' + (' * mo_ir;' if s.compressible else ';'))
    L.append(f'  const {ct} mo_s = drho[rc]' + (' - (' + ' + '.join(
        f'mo_d{a} * vel_out[{_vel(a)}]' for a in range(cx.D)) + ');' if s.compressible else ';'))


def seed(cx, i):
    """`` + seed_i`` after the load of ``g_i``."""
    if not cx.s.mo:
        return ''
    cd = signed_sum(cx, i, 'mo_d')
    return f' + (mo_s + {cd})' if cd else ' + mo_s'


def force_seed(cx, a):
    """Guo with a force field: u reads F directly, ``dforce_a += dvel_a / 2 (/ρ)``."""
    return f' + ({cx.ct})0.5 * mo_d{a}' if cx.s.mo and cx.s.fm == 'guo' else ''
