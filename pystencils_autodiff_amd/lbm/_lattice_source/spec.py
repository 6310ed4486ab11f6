"""What the lattice printer prints: ``LatticeSource`` with its derived facts and refusals, and the boundaries' link
coefficient rows and link programs as named values (the one place that knows the tuples ``boundaries`` returns)."""
from dataclasses import dataclass
from typing import NamedTuple

SELF_BIT = 30      # bit of a cell's neighbour mask: the cell itself is an obstacle (bits 0..Q-1: x − c_i is one)
FIX_BIT = 31       # ... the cell is a fluid cell next to a wall with a link program (the HIP fix-up kernels' cells)
FIX_BLOCK = 64     # threads per workgroup of the fix-up kernel

ARRAYS = dict(s='src', d='dst', g='g', o='out')       # the pdf arrays of the kernels, by the prefix of their strides


def density_links_message(what, who='lattice kernels'):
    """The one wording of the refusal of density-reading links (``what``: 'zero_centered pdfs' / 'float16 pdfs'), here
    and where the step refuses the boundary before any kernel is made."""
    return (f'{who} with {what}: links that read a density (density-weighted links, link programs, neighbour links) '
            'are not built for them')


def _key(d):
    return '_'.join({0: '0', 1: 'm', -1: 'p'}[c] for c in d)      # pull: x − c → m(inus) / p(lus)


class LinkRow(NamedTuple):
    """One direction's link coefficients (``boundaries.link_coefficients``; rows of three have no density terms)."""
    alpha: float
    beta: float
    gamma: float
    beta_rho: float = 0.0
    gamma_rho: float = 0.0

    @property
    def reads_density(self):
        return self.beta_rho != 0 or self.gamma_rho != 0


class JacobianEntry(NamedTuple):
    """``diffpdf[c_offset](component) ← expr · diffpdf[c_d](ī_d)`` (``lines``: the expression's temporaries;
    ``offset``: a direction index, 0 for the cell itself)."""
    component: int
    lines: tuple
    expr: str
    offset: int = 0

    @property
    def own(self):
        """The entry is at the cell itself."""
        return self.offset == 0


class LinkProgram(NamedTuple):
    """One direction's link program (``boundaries.link_program`` / ``neighbour_link_program``): the forward link's
    temporaries and value, its Jacobian entries, and — a neighbour link only, else None — the offsets it reads."""
    lines: tuple
    value: str
    jac: tuple
    reads: object = None

    @property
    def neighbour(self):
        """A neighbour link (``boundaries.neighbour_link_program``'s row form, whatever it reads)."""
        return self.reads is not None


def link_rows(links):
    """``links`` (None, or per wall id the rows of ``boundaries.link_coefficients``) with every row a ``LinkRow``."""
    return None if links is None else tuple(tuple(LinkRow(*(float(v) for v in t)) for t in lk) for lk in links)


def link_programs(programs):
    """``programs`` (per wall id None or per direction None / a program row of three or four) with every row a
    ``LinkProgram`` of ``JacobianEntry``s."""
    def one(row):
        if row is None:
            return None
        lines, value, jac = row[:3]
        return LinkProgram(tuple(lines), value, tuple(JacobianEntry(*r) for r in jac),
                           tuple(row[3]) if len(row) > 3 else None)
    return tuple(None if pg is None else tuple(one(row) for row in pg) for pg in programs or ())


@dataclass(eq=False)
class LatticeSource:
    """What ``emit`` prints.

    ``walls``: a ``uint32`` neighbour mask per cell (bit i: ``x − c_i`` is an obstacle; bit ``SELF_BIT``: ``x`` is
    one), one load per cell.
    ``links``: None (every wall a plain bounce-back), or per wall id (the flag array's values) the boundary's link
    coefficients per direction (``boundaries.link_coefficients``): a bounced component then becomes
    ``α·src_ī(x) + β`` (id of the wall cell ``x − c_i`` from the flag array) and its adjoint is scaled by γ.
    ``programs``: per wall id None or the boundary's link program (the package docstring).
    ``force_model`` 'simple' / 'guo' with a constant body force ``force`` (D numbers, ``_method._force``), or
    (``force_field``, ``force`` unused) a per-cell vector field ``[*domain, D]`` read by strides (an additional input of
    the rule, ``_autodiff_lbstep.py:113-128``).
    ``trt``: the TRT method (``_method.create_lb_update_rule(method='trt')``): ``('magic', Λ)`` (ω₋ from ω and the
    magic number, computed per launch from the ω argument) or ``('rate', ω₋)`` (a constant).
    ``mrt``: the MRT method's relaxation matrix ``A = ω P_ω + C`` (``(P_ω, C)``, Q×Q numbers, ``_method.
    mrt_relaxation_matrices`` summed over the groups relaxing with the ω argument / with constant rates).
    ``omega_field``: the relaxation rate ω is a per-cell scalar field ``[*domain]`` read by strides (the scalar ``omega``
    argument is then ignored) and the adjoint ACCUMULATES ``dω(x) = Σ_i g_i ∂dst_i/∂ω`` into ``domega``
    (``omega.omega_adjoint``).
    ``target`` 'hip' / 'c'. ``idx``: the type of every stride and element offset (``long long`` once an array, or the
    force field, reaches 2³¹ − 1 elements). ``addr`` 'buf' / 'ptr' (``addressing.Addressing``). ``mode`` 'inline' /
    'main' / 'fix' (the package docstring).
    ``half``: the pdf arrays hold IEEE half floats and ``ctype`` (``float``) is the compute type alone: HIP loads and
    stores ``_Float16`` (2-byte buffer accesses), the C target ``uint16_t`` bits through the CPU backend's conversion
    helpers; every store rounds to nearest-even.
    ``zero_centered``: the STATE arrays (``src`` of every kernel, ``dst`` of the forward) hold ``δf_i = f_i − w_i``
    (lbmpy's zero-centred storage, background density 1): every load of a pulled or bounced state value adds ``w_i``
    in the compute type (``w_i = w_ī``, so a bounce-back and the affine links need nothing more), every store of a
    forward result subtracts it before the cast to the storage type. The adjoint arrays ``g`` / ``out`` and the
    obstacle cells' copies are not shifted.
    Links that read a density (density-weighted links, link programs, neighbour links) are printed for plain pdfs of
    the compute type only: with ``zero_centered`` or ``half`` they raise ``NotImplementedError`` (their second pass
    and fix-up launch accumulate in the storage type, and there is no single-half atomic), as do ``half`` force / ω
    fields (the field's adjoint would accumulate over the steps in half precision).
    ``smagorinsky``: None, or the Smagorinsky constant C_s (``_method.create_lb_update_rule(smagorinsky=…)``): the rate
    the collision reads is ``ω_eff = 2 / (τ0 + √(τ0² + 18 C_s² q))`` of the cell's own pulled pdfs, τ0 = 1/ω0 with ω0 the
    ω argument or the ω field's value (``smagorinsky.smagorinsky_rate``), and the adjoint carries the chain factors
    ``∂ω_eff/∂f_k`` on the scatter and ``∂ω_eff/∂ω0`` on ``domega`` (``smagorinsky.smagorinsky_adjoint``). Not printed
    for ``half`` pdfs nor with a per-cell force field (whose adjoint would need ∂ω_eff/∂F): ``NotImplementedError``.
    ``macroscopic``: the forward also writes the density and the velocity of the state it stores, and the adjoint
    takes their adjoint seeds (``macroscopic.py``); off, every source is what it was without the flag, to the byte.
    ``solid_field``: a per-cell solid fraction σ ``[*domain]`` read by strides (partial bounce-back): the forward stores
    ``(1 − σ) c_i + σ f_ī``, the adjoint blends ``v_j`` likewise, scales ``dω`` / ``dF`` by ``1 − σ`` and ACCUMULATES
    ``dσ(x) = Σ_i g_i (f_ī − c_i)`` into ``dsolid`` (``solid.py``); off, no line of any source changes. Not printed
    for ``half`` pdfs (``NotImplementedError``, as the ω field).

    The derived facts below follow from the fields in ``__post_init__``; a variant (another index type, addressing or
    mode) is made with ``dataclasses.replace``, never by assignment."""
    stencil: object
    compressible: bool
    ctype: str
    walls: bool
    links: object = None
    programs: object = None
    force_model: object = None
    force: object = None
    force_field: bool = False
    trt: object = None
    mrt: object = None
    target: str = 'c'
    idx: str = 'i64'
    addr: str = 'ptr'
    mode: str = 'inline'
    omega_field: bool = False
    zero_centered: bool = False
    half: bool = False
    smagorinsky: object = None
    macroscopic: bool = False
    solid_field: bool = False

    def __post_init__(self):
        self.hip, self.fix = self.target == 'hip', self.mode == 'fix'
        self.dirs = [tuple(d) for d in self.stencil.directions]
        self.inv = [self.stencil.inverse_direction_index(i) for i in range(self.stencil.Q)]
        self.axes = ['z', 'y', 'x'][3 - self.stencil.D:]          # spatial axes, axis 0 slowest; x fastest
        self.keys = sorted({_key(d) for d in self.dirs})          # one name per distinct neighbour cell x − c
        self.fm = None if self.force_model is None else str(self.force_model).lower()
        self.ff = bool(self.fm) and bool(self.force_field)
        self.of = bool(self.omega_field)
        self.mo = bool(self.macroscopic)
        self.sf = bool(self.solid_field)
        # Guo with TRT / MRT: the force term (prefactor 1 − ω/2 with the shear rate ω, as lbmpy's Guo model) is not
        # relaxed by the collision matrix, so its adjoint sums run over g while the equilibrium's run over h
        self.sm = None if self.smagorinsky is None else float(self.smagorinsky)
        if self.sm is not None:
            if not self.sm > 0:
                raise ValueError(f'smagorinsky: a positive constant, got {self.smagorinsky!r}')
            if self.half:
                raise NotImplementedError('lattice kernels with smagorinsky: not built for float16 pdfs')
            if self.ff:
                raise NotImplementedError('lattice kernels with smagorinsky: not built with a per-cell force field '
                                          '(its adjoint would need the derivative of the effective rate by the force)')
        # (Smagorinsky: the equilibrium sums of every method run over h_i − λ P_i, ``smagorinsky_adjoint``, so SRT's
        # force term is split off them as well)
        self.gsplit = self.fm == 'guo' and (self.trt is not None or self.mrt is not None or self.sm is not None)
        # the links and programs by name: per wall id the ``LinkRow`` of every direction / None or per direction None
        # or its ``LinkProgram``
        self.link_rows = link_rows(self.links)
        self.progs = link_programs(self.programs)
        # links whose value also depends on the fluid cell's density ρ(x) = Σ_k src_k(x) (a density-weighted moving
        # wall): forward f_j += βρ·ρ(x); the adjoint adds Σ_j βρ_j v_j to every component of the cell in a second pass
        self.rho_links = self.links is not None and any(t.beta_rho != 0 for lk in self.link_rows for t in lk)
        self.gen = self.links is not None and any(p is not None for p in self.progs)
        self.inl = self.gen and self.mode == 'inline'
        # the adjoint's second pass over a per-cell scratch array: density-weighted links (any mode), link programs
        # inline
        self.two = self.rho_links or self.inl
        # (direction, program) of every link program
        prows = [(d, pg) for wall in self.progs if wall is not None for d, pg in enumerate(wall) if pg is not None] \
            if self.gen else []
        # neighbour links (``boundaries.neighbour_link_program``: Jacobian entries with an offset index)
        self.nb = any(pg.neighbour for _, pg in prows)
        # the components q of a listed cell x that receive G_q = Σ_j J_jq v_j (link programs' Jacobian columns) plus,
        # for neighbour links, the components they add into at the cells they read and the link's own direction d
        # (the entry the replaced bounce-back would have written: zeroed, it receives adds only)
        self.gq_all = sorted({r.component for _, pg in prows for r in pg.jac} | {d for d, pg in prows if pg.neighbour})
        # the components with Jacobian entries at the cell itself (the G accumulators)
        self.g_own = sorted({r.component for _, pg in prows for r in pg.jac if r.own})
        self.zc, self.h = bool(self.zero_centered), bool(self.half)
        for on, what in ((self.zc, 'zero_centered pdfs'), (self.h, 'float16 pdfs')):
            if on and (self.rho_links or self.gen):
                raise NotImplementedError(density_links_message(what))
        if self.h and (self.ff or self.of):
            raise NotImplementedError('lattice kernels for float16 pdfs: a per-cell force / relaxation-rate field is '
                                      'not built (its adjoint would accumulate in float16)')
        if self.h and self.sf:
            raise NotImplementedError('lattice kernels for float16 pdfs: a per-cell solid-fraction field is '
                                      'not built (its adjoint would accumulate in float16)')
