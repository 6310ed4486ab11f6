"""The printers' shared context (one per module printed) and the small expressions every part uses. Every printer is a
plain function over the context ``cx``: it appends lines to ``L`` or returns an expression."""
from .addressing import Addressing
from .args import KERNELS, kernel_args, rate_names
from .spec import _key


def _c(v):
    """A rational / float constant as a C literal of the compute type."""
    return repr(float(v))


class Context:
    """What the parts of one module's text share: the spec ``s``, its addressing ``A`` and the facts derived once."""

    def __init__(self, spec):
        s = self.s = spec
        if s.mrt is not None and s.trt is not None:
            raise NotImplementedError('MRT and TRT lattice kernels at once')
        if s.fix and not s.gen:
            raise ValueError('fix-up kernels need link programs')
        self.A = Addressing(s)
        self.D, self.Q, self.ct = s.stencil.D, s.stencil.Q, s.ctype
        self.dirs, self.inv, self.axes = s.dirs, s.inv, s.axes
        self.w = [float(x) for x in s.stencil.weights]
        self.F = [float(v) for v in s.force] if s.fm and not s.ff else None
        self.cF = [sum(c * f for c, f in zip(d, self.F)) for d in self.dirs] if self.F is not None else None
        self.centre = '_'.join('0' for _ in self.axes)
        self.low = f'{(1 << self.Q) - 1}u'                 # neighbour-mask bits of the Q directions
        self.cell = '((IDX)z * Y + y) * X + x' if self.D == 3 else '(IDX)y * X + x'
        self.ncells = '(IDX)Z * Y * X'
        self.fn = '__device__ static inline' if s.hip else 'static inline'
        self.adj_progs = s.gen and s.mode != 'main'     # the main HIP adjoint leaves the program cells to the fix-up
        # the rate: the scalar argument (unused with an ω field, which the cell loads), the cell's ω0 and — the name the
        # collision reads — ``omega`` (Smagorinsky: the effective rate, computed from ω0 in ``moments``)
        self.om0, self.om_arg = rate_names(s)
        # ``sig`` / ``args``: the parameter lists of the cell functions ``lbm_{fwd,adj,adj_rho}_cell`` (and of the HIP
        # kernels) and the matching argument lists
        self.tables = {k: kernel_args(s, k) for k in KERNELS}
        self.sig = {k: ', '.join(a.decl for a in t) for k, t in self.tables.items()}
        self.args = {k: ', '.join(a.name for a in t) for k, t in self.tables.items()}
        self.fstr_unused = '(void)f_z; ' if s.ff and self.D == 2 else ''
        if s.of:
            self.fstr_unused += '(void)omega_s; ' + ('(void)w_z; ' if self.D == 2 else '')
        if s.sf and self.D == 2:
            self.fstr_unused += '(void)p_z; '


def c_(cx, v):
    return f'({cx.ct}){_c(v)}'


def signed_sum(cx, i, name, paren=True):
    """``± name_a`` over the nonzero axes of direction i (None for the rest direction)."""
    t = ' '.join(('+ ' if c > 0 else '- ') + f'{name}{a}' for a, c in enumerate(cx.dirs[i]) if c)
    if not t:
        return None
    return t[2:] if t.startswith('+ ') else f'({t})' if paren else t


def axis_sums(cx, L, i, name, t):
    """``name_a ±= t`` over the nonzero axes of direction i."""
    for a, c in enumerate(cx.dirs[i]):
        if c:
            L.append(f'    {name}{a} {"+" if c > 0 else "-"}= {t};')


def cu_poly(cx, L, i, poly=True):
    """Opens the block of direction i: ``cu`` = c_i·u and the equilibrium's polynomial in it."""
    ct = cx.ct
    L.append(f'  {{ const {ct} cu = {signed_sum(cx, i, "u") or f"({ct})0"};')
    if poly:
        L.append(f'    const {ct} poly = cu * (({ct})3 + ({ct})4.5 * cu) - ({ct})1.5 * usq;')


def feq(cx, i):
    """The equilibrium of direction i (after ``cu_poly``): w_i ρ (1 + 3 c_i·u + 4.5 (c_i·u)² − 1.5 u²), the
    incompressible one w_i (ρ + …)."""
    return (f'{c_(cx, cx.w[i])} * rho * (({cx.ct})1 + poly)' if cx.s.compressible
            else f'{c_(cx, cx.w[i])} * (rho + poly)')


def shift(cx, i, sign=' + '):
    """Zero-centred pdfs: `` + w_i`` after a load of a state value, `` - w_i`` before a forward result's store."""
    return f'{sign}{c_(cx, cx.w[i])}' if cx.s.zc else ''


def mat_row(cx, M, vec, i, transpose=False):
    """Σ_k M[i][k] vec_k (or M[k][i]) as C, zero entries left out (None when the row is all zeros)."""
    row = [float(M[k][i] if transpose else M[i][k]) for k in range(cx.Q)]
    return ' + '.join(f'{c_(cx, v)} * {vec}{k}' for k, v in enumerate(row) if v != 0.0) or None


def Fa(cx, a):
    """Force component a: a constant, or the cell's value (``force_field``)."""
    return f'F{a}' if cx.s.ff else c_(cx, cx.F[a])


def cFi(cx, i, scale=1):
    """scale · (c_i · F) (None where it is the constant 0)."""
    if cx.s.ff:
        if not any(cx.dirs[i]):
            return None
        return f'cF{i}' if scale == 1 else f'({c_(cx, scale)} * cF{i})'
    return c_(cx, scale * cx.cF[i]) if cx.cF[i] else None


def ncell(cx, k):
    """C-order cell index of the neighbour ``x − c`` of pull key ``k`` (wrapped coordinates)."""
    co = cx.A.coord
    if cx.D == 3:
        return f'((IDX){co(k, "z")} * Y + {co(k, "y")}) * X + {co(k, "x")}'
    return f'(IDX){co(k, "y")} * X + {co(k, "x")}'


def key(cx, i):
    """The pull key of direction i's neighbour cell ``x − c_i``."""
    return _key(cx.dirs[i])
