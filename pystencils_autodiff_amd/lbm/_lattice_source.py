"""The text of the lattice Boltzmann kernels (``_lattice_kernels`` compiles and launches them).

``LatticeSource`` says what to print — the lattice (stencil, collision, force, walls and their links), the target
(HIP / C), the index type, the addressing mode and the adjoint mode — and ``emit`` prints it: the forward cell
(``lbm_fwd_cell``), the adjoint cell (``lbm_adj_cell``: prologue, moment-like sums, force adjoint, ω-field adjoint,
scatter), the adjoint's second pass (``lbm_adj_rho_cell``) and the entry points that call them for every cell: HIP
grid kernels, the HIP fix-up kernel over a cell list, or C loop nests.

Adjoint modes. ``programs`` gives per wall id None or the boundary's ``link_program`` (links of the cell's own pdfs the
fused form does not take, ``boundaries.link_program``; their table rows are zeros): the forward evaluates the link
from the cell's own pdfs ``c0 … c{Q-1}`` (loaded inside the link's branch), the adjoint's first pass stores ``v_j`` of
each program-linked component j to a per-cell scratch array and the second pass (``lbm_adj_rho``) adds
``Σ_j J_jk(c) v_j`` to component k of the cell — the Jacobians are evaluated there, on the cells next to a wall, not in
the first pass, whose registers they would take on every cell (``mode='inline'``, the C target).
HIP (``mode='main'`` / ``'fix'``): the forward evaluates the programs inline as above; the main adjoint carries no
program code and leaves the cells marked ``FIX_BIT`` (fluid cells next to a program wall) to ONE list-driven fix-up
kernel (``lbm_adj_fix``): the regular scatter plus ``out_k(x) += G_k``, ``G_k = Σ_j J_jk v_j`` (``_Printer.prologue``
and ``_Printer.scatter_store`` have the protocol of the two launches). The lattice's bulk runs the plain adjoint
(measured: profiles/r05_lbm_pressure.jsonl, r06_lbm_fix_merge.jsonl).
"""
import re
from dataclasses import dataclass

SELF_BIT = 30      # bit of a cell's neighbour mask: the cell itself is an obstacle (bits 0..Q-1: x − c_i is one)
FIX_BIT = 31       # ... the cell is a fluid cell next to a wall with a link program (the HIP fix-up kernels' cells)
FIX_BLOCK = 64     # threads per workgroup of the fix-up kernel

ARRAYS = dict(s='src', d='dst', g='g', o='out')       # the pdf arrays of the kernels, by the prefix of their strides


def density_links_message(what, who='lattice kernels'):
    """The one wording of the refusal of density-reading links (``what``: 'zero_centered pdfs' / 'float16 pdfs'), here
    and where the step refuses the boundary before any kernel is made."""
    return (f'{who} with {what}: links that read a density (density-weighted links, link programs, neighbour links) '
            'are not built for them')


def _c(v):
    """A rational / float constant as a C literal of the compute type."""
    return repr(float(v))


def _key(d):
    return '_'.join({0: '0', 1: 'm', -1: 'p'}[c] for c in d)      # pull: x − c → m(inus) / p(lus)


@dataclass(eq=False)
class LatticeSource:
    """What ``emit`` prints.

    ``walls``: a ``uint32`` neighbour mask per cell (bit i: ``x − c_i`` is an obstacle; bit ``SELF_BIT``: ``x`` is
    one), one load per cell.
    ``links``: None (every wall a plain bounce-back), or per wall id (the flag array's values) the boundary's link
    coefficients per direction (``boundaries.link_coefficients``): a bounced component then becomes
    ``α·src_ī(x) + β`` (id of the wall cell ``x − c_i`` from the flag array) and its adjoint is scaled by γ.
    ``programs``: per wall id None or the boundary's link program (the module docstring).
    ``force_model`` 'simple' / 'guo' with a constant body force ``force`` (D numbers, ``_method._force``), or
    (``force_field``, ``force`` unused) a per-cell vector field ``[*domain, D]`` read by strides (an additional input of
    the rule, ``_autodiff_lbstep.py:113-128``).
    ``trt``: the TRT method (``_method.create_lb_update_rule(method='trt')``): ``('magic', Λ)`` (ω₋ from ω and the
    magic number, computed per launch from the ω argument) or ``('rate', ω₋)`` (a constant).
    ``mrt``: the MRT method's relaxation matrix ``A = ω P_ω + C`` (``(P_ω, C)``, Q×Q numbers, ``_method.
    mrt_relaxation_matrices`` summed over the groups relaxing with the ω argument / with constant rates).
    ``omega_field``: the relaxation rate ω is a per-cell scalar field ``[*domain]`` read by strides (the scalar ``omega``
    argument is then ignored) and the adjoint ACCUMULATES ``dω(x) = Σ_i g_i ∂dst_i/∂ω`` into ``domega``
    (``_Printer.omega_adjoint``).
    ``target`` 'hip' / 'c'. ``idx``: the type of every stride and element offset (``long long`` once an array, or the
    force field, reaches 2³¹ − 1 elements). ``addr`` 'buf' / 'ptr' (``_Addressing``). ``mode`` 'inline' / 'main' /
    'fix' (the module docstring).
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
    ω argument or the ω field's value (``_Printer.smagorinsky_rate``), and the adjoint carries the chain factors
    ``∂ω_eff/∂f_k`` on the scatter and ``∂ω_eff/∂ω0`` on ``domega`` (``_Printer.smagorinsky_adjoint``). Not printed
    for ``half`` pdfs nor with a per-cell force field (whose adjoint would need ∂ω_eff/∂F): ``NotImplementedError``.

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

    def __post_init__(self):
        links, programs = self.links, self.programs
        self.hip, self.fix = self.target == 'hip', self.mode == 'fix'
        self.dirs = [tuple(d) for d in self.stencil.directions]
        self.inv = [self.stencil.inverse_direction_index(i) for i in range(self.stencil.Q)]
        self.axes = ['z', 'y', 'x'][3 - self.stencil.D:]          # spatial axes, axis 0 slowest; x fastest
        self.keys = sorted({_key(d) for d in self.dirs})          # one name per distinct neighbour cell x − c
        self.fm = None if self.force_model is None else str(self.force_model).lower()
        self.ff = bool(self.fm) and bool(self.force_field)
        self.of = bool(self.omega_field)
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
        # links whose value also depends on the fluid cell's density ρ(x) = Σ_k src_k(x) (a density-weighted moving
        # wall): forward f_j += βρ·ρ(x); the adjoint adds Σ_j βρ_j v_j to every component of the cell in a second pass
        self.rho_links = links is not None and any(len(t) > 3 and t[3] != 0 for lk in links for t in lk)
        self.gen = links is not None and programs is not None and any(p is not None for p in programs)
        self.inl = self.gen and self.mode == 'inline'
        # the adjoint's second pass over a per-cell scratch array: density-weighted links (any mode), link programs
        # inline
        self.two = self.rho_links or self.inl
        # (direction, program row) of every link program
        prows = [(d, row) for pg in programs if pg is not None for d, row in enumerate(pg) if row is not None] \
            if self.gen else []
        # neighbour links (``boundaries.neighbour_link_program``: rows of four, Jacobian entries with an offset index)
        self.nb = any(len(row) > 3 for _, row in prows)
        # the components q of a listed cell x that receive G_q = Σ_j J_jq v_j (link programs' Jacobian columns) plus,
        # for neighbour links, the components they add into at the cells they read and the link's own direction d
        # (the entry the replaced bounce-back would have written: zeroed, it receives adds only)
        self.gq_all = sorted({r[0] for _, row in prows for r in row[2]} | {d for d, row in prows if len(row) > 3})
        # the components with Jacobian entries at the cell itself (the G accumulators)
        self.g_own = sorted({r[0] for _, row in prows for r in row[2] if len(r) < 4 or r[3] == 0})
        self.zc, self.h = bool(self.zero_centered), bool(self.half)
        for on, what in ((self.zc, 'zero_centered pdfs'), (self.h, 'float16 pdfs')):
            if on and (self.rho_links or self.gen):
                raise NotImplementedError(density_links_message(what))
        if self.h and (self.ff or self.of):
            raise NotImplementedError('lattice kernels for float16 pdfs: a per-cell force / relaxation-rate field is '
                                      'not built (its adjoint would accumulate in float16)')


class _Addressing:
    """How the kernels reach the pdf arrays ``src`` / ``dst`` / ``g`` / ``out`` (prefixes s, d, g, o of ``ARRAYS``).

    ``'buf'`` (HIP): every pdf array is one buffer resource (its bytes below 2³¹: the record count and the
    components' scalar offsets pass through ``int``); a component's plane offset ``q·s_q`` rides in the instruction's
    scalar offset and each distinct neighbour cell's byte offset is ONE 32-bit VGPR shared by all components that pull
    from it — no 64-bit address arithmetic per access. ``'ptr'``: plain pointers and element offsets of type IDX (the C
    target, and arrays of 2 GiB and more: ``LatticeKernels._mode`` switches at 2³¹ bytes)."""

    def __init__(self, spec):
        self.buf = spec.hip and spec.addr == 'buf'
        self.ct, self.axes, self.keys = spec.ctype, spec.axes, spec.keys
        self.esize = 2 if spec.h else 8 if spec.ctype == 'double' else 4
        self.bits, self.ty = {8: ('b64', 'u32x2'), 4: ('b32', 'unsigned'), 2: ('b16', 'unsigned short')}[self.esize]
        self.half, self.chalf = spec.h, spec.h and not spec.hip       # (C: uint16_t bits and conversion helpers)
        self.off_type = 'unsigned' if self.buf else 'IDX'      # of a cell's (byte / element) offset

    def coord(self, k, a):
        c = k.split('_')[self.axes.index(a)]
        return a if c == '0' else f'{a}{c}'

    def resource(self, L, p):
        """The resource descriptor of array ``p`` and its plane stride in bytes."""
        if self.buf:
            L.append(f'  const __amdgpu_buffer_rsrc_t rs_{p} = __builtin_amdgcn_make_buffer_rsrc((void*){ARRAYS[p]}, '
                     f'(short)0, (int){p}_bytes, 0x00020000);')
            L.append(f'  const int {p}_qb = (int){p}_q * {self.esize};')

    def neighbour_offsets(self, L, p):
        """``{p}o_{key}``: one element (ptr) or byte (buf) offset per distinct neighbour cell of array ``p``."""
        for k in self.keys:
            e = ' + '.join(f'(IDX){self.coord(k, a)} * {p}_{a}' for a in self.axes)
            if self.buf:
                L.append(f'  const unsigned {p}o_{k} = (unsigned)({e}) * {self.esize}u;')
            else:
                L.append(f'  const IDX {p}o_{k} = {e};')

    def cell_offset(self, L, p):
        """The cell's own offset in array ``p`` (which has no neighbour offsets); returns its name."""
        L.append(_cell_offset(p, self.axes))
        if self.buf:
            L.append(f'  const unsigned {p}cb = (unsigned){p}c * {self.esize}u;')
        return f'{p}cb' if self.buf else f'{p}c'

    def _rd(self, e):
        """The element ``e`` of a pdf array as a value (half floats: converted to the compute type)."""
        return f'({self.ct})psad_h2f({e})' if self.chalf else f'({self.ct}){e}' if self.half else e

    def _wr(self, val, paren=True):
        """``val`` in the storage type (half floats on the C target: rounded to nearest-even by the helper)."""
        if self.chalf:
            return f'psad_f2h((float)({val}))'
        return f'(T)({val})' if paren else f'(T){val}'

    def load(self, p, comp, off):
        """Component ``comp`` (a constant: its plane offset is a scalar) at cell offset ``off``."""
        if self.buf:
            return self._buffer_load(p, off, f'{comp} * {p}_qb')
        # (always cast, as this load always was; ``_rd`` casts half floats only: the loads that go through it alone —
        # ``load_v``, ``select_load`` — had no cast, and the plain sources stay what they were, to the byte)
        e = f'{ARRAYS[p]}[(IDX){comp} * {p}_q + {off}]'
        return self._rd(e) if self.chalf else f'({self.ct}){e}'

    def copy(self, p, comp, off, sp, soff):
        """``p[comp, off] = sp[comp, soff]`` as the stored bits, never converted (half floats: an obstacle cell's
        copy keeps NaN payloads too)."""
        if self.buf:
            return (f'__builtin_amdgcn_raw_buffer_store_{self.bits}(__builtin_amdgcn_raw_buffer_load_{self.bits}('
                    f'rs_{sp}, {soff}, {comp} * {sp}_qb, 0), rs_{p}, {off}, {comp} * {p}_qb, 0);')
        return f'{ARRAYS[p]}[(IDX){comp} * {p}_q + {off}] = {ARRAYS[sp]}[(IDX){comp} * {sp}_q + {soff}];'

    def store(self, p, comp, off, val):
        if self.buf:
            return self._buffer_store(p, off, f'{comp} * {p}_qb', val)
        return f'{ARRAYS[p]}[(IDX){comp} * {p}_q + {off}] = {self._wr(val)};'

    def lane(self, p, comp, k):
        """The per-lane offset of (component, neighbour cell ``k``): the plane offset folded in."""
        return f'{p}o_{k} + (unsigned)({comp} * {p}_qb)' if self.buf else f'(IDX){comp} * {p}_q + {p}o_{k}'

    def load_v(self, p, voff):
        """One load at a per-lane offset (``lane``; no scalar offset)."""
        return self._buffer_load(p, voff, '0') if self.buf else self._rd(f'{ARRAYS[p]}[{voff}]')

    def store_v(self, p, voff, val):
        """One store of the variable ``val`` at a per-lane offset."""
        return self._buffer_store(p, voff, '0', val) if self.buf else \
            f'{ARRAYS[p]}[{voff}] = {self._wr(val, paren=False)};'

    def select_load(self, L, decl, p, bit, bounced, pulled, shift=''):
        """``decl = msk bit ? array[bounced] : array[pulled]`` (lane offsets) as ONE load whose per-lane offset
        selects (component, cell) — not both loads and a select. ``shift``: the `` + w`` of zero-centred pdfs."""
        if self.buf:
            L.append(f'  const unsigned vo{bit} = ((msk >> {bit}) & 1u) ? {bounced} : {pulled};')
            L.append(f'  {decl} = {self.load_v(p, f"vo{bit}")}{shift};')
        else:
            L.append(f'  {decl} = ' + self._rd(f'{ARRAYS[p]}[(msk >> {bit}) & 1u ? {bounced} : {pulled}]') +
                     f'{shift};')

    def select_store(self, L, p, bit, bounced, pulled, val):
        """The store likewise (closes the block of the component)."""
        if self.buf:
            L.append(f'    const unsigned vs = ((msk >> {bit}) & 1u) ? {bounced} : {pulled};')
            L.append(f'    {self.store_v(p, "vs", val)} }}')
        else:
            L.append(f'    {ARRAYS[p]}[(msk >> {bit}) & 1u ? {bounced} : {pulled}] = '
                     f'{self._wr(val, paren=False)}; }}')

    def atomic_add(self, voff, val):
        """``out[voff] += val`` atomically (``voff``: a lane offset)."""
        return f'atomicAdd({f"(T*)((char*)out + {voff})" if self.buf else f"out + {voff}"}, {val});'

    def _buffer_load(self, p, voff, soff):
        return (f'({self.ct})__builtin_bit_cast(T, ({self.ty})__builtin_amdgcn_raw_buffer_load_{self.bits}('
                f'rs_{p}, {voff}, {soff}, 0))')

    def _buffer_store(self, p, voff, soff, val):
        return (f'__builtin_amdgcn_raw_buffer_store_{self.bits}(__builtin_bit_cast({self.ty}, (T)({val})), rs_{p}, '
                f'{voff}, {soff}, 0);')


def _cell_offset(p, axes):
    return f'  const IDX {p}c = ' + ' + '.join(f'(IDX){a} * {p}_{a}' for a in axes) + ';'


def _wrap_lines(L, axes):
    """The periodic neighbours' coordinates."""
    for a in axes:
        N = a.upper()
        L.append(f'  const int {a}m = {a} == 0 ? {N} - 1 : {a} - 1, {a}p = {a} == {N} - 1 ? 0 : {a} + 1;')


C_LOOPS = ('  #pragma omp parallel for collapse(2) schedule(static)\n'
           '  for (int z = 0; z < Z; ++z)\n    for (int y = 0; y < Y; ++y)\n      for (int x = 0; x < X; ++x)')
CELL_ZYX = ('  const unsigned r = cell / (unsigned)X;\n'
            '  const int x = (int)(cell - r * (unsigned)X);\n'
            '  const int z = (int)(r / (unsigned)Y), y = (int)(r - (unsigned)z * Y);')


def emit(spec):
    """Source of the forward (``lbm_fwd``) and adjoint (``lbm_adj``) kernels of ``spec`` (a ``LatticeSource``)."""
    return _Printer(spec).module()


class _Printer:
    """The parts of one module's text; every method appends lines to ``L`` or returns an expression."""

    def __init__(self, spec):
        s = self.s = spec
        if s.mrt is not None and s.trt is not None:
            raise NotImplementedError('MRT and TRT lattice kernels at once')
        if s.fix and not s.gen:
            raise ValueError('fix-up kernels need link programs')
        self.A = _Addressing(s)
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
        self.om0 = 'omega_0' if s.sm is not None else 'omega'
        self.om_arg = 'omega_s' if s.of else self.om0
        self._signatures()

    def _signatures(self):
        """``sig`` / ``args``: the parameter lists of the cell functions ``lbm_{fwd,adj,adj_rho}_cell`` (and of the HIP
        kernels) and the matching argument lists."""
        s = self.s

        def params(pdfs, more):
            """Of the cell function over the pdf arrays ``pdfs`` (the last one written)."""
            P = [f'const T* __restrict__ {ARRAYS[p]}' for p in pdfs[:-1]] + [f'T* __restrict__ {ARRAYS[pdfs[-1]]}']
            P += ['const unsigned* __restrict__ nbmask', 'const unsigned char* __restrict__ wallid'] + more
            P += ['const int Z', 'const int Y', 'const int X'] + [f'const IDX {p}_{a}' for p in pdfs for a in 'qzyx']
            P += [f'const IDX f_{a}' for a in 'czyx'] if s.ff else []
            P += [f'const IDX w_{a}' for a in 'zyx'] if s.of else []
            # (with an ω field the scalar rate is not what the collision reads: the cell loads ``omega``)
            return P + [f'const long long {p}_bytes' for p in pdfs] + [f'const {self.ct} {self.om_arg}']
        force = ['const T* __restrict__ force'] if s.ff else []
        omf = ['const T* __restrict__ omf'] if s.of else []
        rho = ['T* __restrict__ out', 'const unsigned* __restrict__ nbmask', 'const T* __restrict__ rho_adj',
               'const int Z', 'const int Y', 'const int X'] + [f'const IDX o_{a}' for a in 'qzyx']
        if s.inl:
            # the programs' Jacobians read the cell's own pdfs and the neighbours' wall ids
            rho += ['const T* __restrict__ src', 'const unsigned char* __restrict__ wallid'] + \
                [f'const IDX s_{a}' for a in 'qzyx']
        P = dict(fwd=params('sd', force + omf), adj_rho=rho,
                 adj=params('sgo', force + (['T* __restrict__ dforce'] if s.ff else []) +
                            omf + (['T* __restrict__ domega'] if s.of else []) +
                            (['T* __restrict__ rho_adj'] if s.two else [])))
        self.sig = {k: ', '.join(v) for k, v in P.items()}
        self.args = {k: ', '.join(p.split()[-1] for p in v) for k, v in P.items()}
        self.fstr_unused = '(void)f_z; ' if s.ff and self.D == 2 else ''
        if s.of:
            self.fstr_unused += '(void)omega_s; ' + ('(void)w_z; ' if self.D == 2 else '')

    def module(self):
        s, L = self.s, []
        if not s.hip:
            L.append('#include <stdint.h>\ntypedef long long i64;')
        if s.h and not s.hip:
            # the pdf arrays hold the half floats' bits: the CPU backend's conversion helpers
            from ..backends.cpu_kernel import _HALF_HELPERS
            L.append('#include <string.h>' + _HALF_HELPERS.rstrip('\n'))
        L.append(f'typedef {("_Float16" if s.hip else "uint16_t") if s.h else s.ctype} T;\ntypedef {s.idx} IDX;')
        if s.hip:
            L.append('typedef unsigned u32x2 __attribute__((ext_vector_type(2)));')
        self.link_tables(L)
        self.smagorinsky_rate(L)
        self.forward_cell(L)
        self.adjoint_cell(L)
        if s.two:
            self.rho_cell(L)
        (self.c_entries if not s.hip else self.hip_fix_entry if s.fix else self.hip_grid_entries)(L)
        return '\n'.join(L) + '\n'

    # ---- small expressions
    def c_(self, v):
        return f'({self.ct}){_c(v)}'

    def signed_sum(self, i, name, paren=True):
        """``± name_a`` over the nonzero axes of direction i (None for the rest direction)."""
        t = ' '.join(('+ ' if c > 0 else '- ') + f'{name}{a}' for a, c in enumerate(self.dirs[i]) if c)
        if not t:
            return None
        return t[2:] if t.startswith('+ ') else f'({t})' if paren else t

    def axis_sums(self, L, i, name, t):
        """``name_a ±= t`` over the nonzero axes of direction i."""
        for a, c in enumerate(self.dirs[i]):
            if c:
                L.append(f'    {name}{a} {"+" if c > 0 else "-"}= {t};')

    def cu_poly(self, L, i, poly=True):
        """Opens the block of direction i: ``cu`` = c_i·u and the equilibrium's polynomial in it."""
        ct = self.ct
        L.append(f'  {{ const {ct} cu = {self.signed_sum(i, "u") or f"({ct})0"};')
        if poly:
            L.append(f'    const {ct} poly = cu * (({ct})3 + ({ct})4.5 * cu) - ({ct})1.5 * usq;')

    def feq(self, i):
        """The equilibrium of direction i (after ``cu_poly``): w_i ρ (1 + 3 c_i·u + 4.5 (c_i·u)² − 1.5 u²), the
        incompressible one w_i (ρ + …)."""
        return (f'{self.c_(self.w[i])} * rho * (({self.ct})1 + poly)' if self.s.compressible
                else f'{self.c_(self.w[i])} * (rho + poly)')

    def shift(self, i, sign=' + '):
        """Zero-centred pdfs: `` + w_i`` after a load of a state value, `` - w_i`` before a forward result's store."""
        return f'{sign}{self.c_(self.w[i])}' if self.s.zc else ''

    def mat_row(self, M, vec, i, transpose=False):
        """Σ_k M[i][k] vec_k (or M[k][i]) as C, zero entries left out (None when the row is all zeros)."""
        row = [float(M[k][i] if transpose else M[i][k]) for k in range(self.Q)]
        return ' + '.join(f'{self.c_(v)} * {vec}{k}' for k, v in enumerate(row) if v != 0.0) or None

    def Fa(self, a):
        """Force component a: a constant, or the cell's value (``force_field``)."""
        return f'F{a}' if self.s.ff else self.c_(self.F[a])

    def cFi(self, i, scale=1):
        """scale · (c_i · F) (None where it is the constant 0)."""
        if self.s.ff:
            if not any(self.dirs[i]):
                return None
            return f'cF{i}' if scale == 1 else f'({self.c_(scale)} * cF{i})'
        return self.c_(scale * self.cF[i]) if self.cF[i] else None

    def ncell(self, k):
        """C-order cell index of the neighbour ``x − c`` of pull key ``k`` (wrapped coordinates)."""
        co = self.A.coord
        if self.D == 3:
            return f'((IDX){co(k, "z")} * Y + {co(k, "y")}) * X + {co(k, "x")}'
        return f'(IDX){co(k, "y")} * X + {co(k, "x")}'

    # ---- link programs
    def omask(self, pg):
        """Mask bits of the cells a neighbour link reads (bit ī_o of a cell's mask: x + c_o is a wall — the same
        fact as that cell's own ``SELF_BIT``, without loading its mask word)."""
        return f'{sum(1 << self.inv[o] for o in pg[3])}u'

    def okey(self, o):
        return _key(self.dirs[self.inv[o]])                    # x + c_o = x − c_ī(o)

    def nb_loads(self, code, rd):
        """Loads of the neighbours' pdfs a program's code reads (``const T n<o>_<k> = src_k(x + c_o);``)."""
        used = sorted({(int(o), int(k)) for o, k in re.findall(r'\bn(\d+)_(\d+)\b', code)})
        return ' '.join(f'const {self.ct} n{o}_{k} = {rd(k, self.okey(o))};' for o, k in used)

    def own_loads(self, code, rd):
        """Loads of the cell's own pdfs a program's code reads (``const T c<q> = …;``; ``rd(q)``: the load)."""
        used = sorted({int(m) for m in re.findall(r'\bc(\d+)\b', code)})
        return ' '.join(f'const {self.ct} c{q} = {rd(q)};' for q in used)

    def program_cases(self, i):
        """(wall id, program of the link pulled as component i: direction ī) for the ids with link programs."""
        if not self.s.gen or not any(self.dirs[i]):
            return []
        ii = self.inv[i]
        return [(wid, pg[ii]) for wid, pg in enumerate(self.s.programs) if pg is not None and pg[ii] is not None]

    # ---- parts shared by the forward and the adjoint cell
    def link_tables(self, L):
        """Per (wall id, pulled component j): the link of direction d = ī_j (the population that left x towards the
        wall cell x + c_d = x − c_j comes back as j)."""
        s, Q = self.s, self.Q
        if s.links is None:
            return
        # (half pdfs: the coefficients stay in the compute type)
        qual = ('__constant__ ' if s.hip else 'static const ') + (self.ct if s.h else 'T')
        cols = (('lk_a', 0), ('lk_b', 1), ('lk_g', 2)) + ((('lk_r', 3), ('lk_gr', 4)) if s.rho_links else ())
        for nm, col in cols:
            vals = [repr(float(s.links[k][self.inv[j]][col] if col < len(s.links[k][self.inv[j]]) else 0.0))
                    for k in range(len(s.links)) for j in range(Q)]
            L.append(f'{qual} {nm}[{len(vals)}] = {{{", ".join(vals)}}};')

    def force_loads(self, L):
        """The cell's force vector and its projections c_i · F (``force_field``)."""
        if not self.s.ff:
            return
        ct = self.ct
        fcell = ' + '.join(f'(IDX){a} * f_{a}' for a in self.axes)
        L.append(f'  const IDX fc = {fcell};')
        for a in range(self.D):
            L.append(f'  const {ct} F{a} = ({ct})force[(IDX){a} * f_c + fc];')
        for i in range(self.Q):
            if any(self.dirs[i]):
                L.append(f'  const {ct} cF{i} = {self.signed_sum(i, "F")};')

    def omega_load(self, L):
        """The cell's relaxation rate (``omega_field``): every use of ``omega`` after it — the collision, the TRT
        rates, Guo's 1 − ω/2, MRT's ω P_ω — reads this local."""
        if not self.s.of:
            return
        L.append('  const IDX wc = ' + ' + '.join(f'(IDX){a} * w_{a}' for a in self.axes) + ';')
        L.append(f'  const {self.ct} {self.om0} = ({self.ct})omf[wc];')

    def pull_loads(self, L, progs=True, hoisted=False):
        """``f_i``: the pulled pdfs of the cell — ``src_i(x − c_i)``, or the link of the wall cell there (bounce-back
        ``src_ī(x)``, its table row ``α f + β (+ βρ ρ)``, or its program).
        ``hoisted`` (the fix-up kernel, whose every cell has program links): the wall ids are loaded for every
        direction up front and the cell's own pdfs ``c<q>`` are already loaded, so no load waits on the mask."""
        s, A, ct, Q, centre = self.s, self.A, self.ct, self.Q, self.centre
        for i in range(Q):
            k = _key(self.dirs[i])
            if not (s.walls and any(self.dirs[i])):
                L.append(f'  const {ct} f{i} = {A.load("s", i, f"so_{k}")}{self.shift(i)};')
                continue
            cq = '' if s.links is not None else 'const '
            bounced, pulled = A.lane('s', self.inv[i], centre), A.lane('s', i, k)
            if hoisted and A.buf:
                # (fix-up kernel: both candidates loaded, then selected — no load waits on the mask)
                L.append(f'  const {ct} fb{i} = {A.load_v("s", bounced)}, fs{i} = {A.load_v("s", pulled)};')
                L.append(f'  {cq}{ct} f{i} = ((msk >> {i}) & 1u) ? fb{i} : fs{i};')
            else:
                # a bounced component is read from the cell itself
                A.select_load(L, f'{cq}{ct} f{i}', 's', i, bounced, pulled, self.shift(i))
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
                L.append(f'  if ((msk >> {i}) & 1u) {{ id{i} = wallid[{self.ncell(k)}]; {link} }}')
            cases = self.program_cases(i) if progs else []
            if cases:
                L.append(f'  if ((msk >> {i}) & 1u) switch (id{i}) {{')
                for wid, pg in cases:
                    body = ' '.join(pg[0]) + f' f{i} = {pg[1]};'
                    ld = '' if hoisted else self.own_loads(body, lambda q: A.load('s', q, f'so_{centre}'))
                    if len(pg) > 3:
                        # a neighbour link: taken where every cell it reads is fluid, else f_i stays the
                        # bounce-back the table row (1, 0) made
                        nl = self.nb_loads(body, lambda q, kk: A.load('s', q, f'so_{kk}'))
                        L.append(f'    case {wid}: if (!(msk & {self.omask(pg)})) {{ {ld} {nl} {body} }} break;')
                    else:
                        L.append(f'    case {wid}: {{ {ld} {body} }} break;')
                L.append('    default: break;\n  }')

    def cell_density(self, L):
        """ρ(x) of the cell's own (pre-streaming) pdfs, for density-weighted links, on cells next to a wall."""
        if not self.s.rho_links:
            return
        L.append(f'  {self.ct} rs = 0;')
        L.append(f'  if (msk & {self.low}) rs = ' + ' + '.join(self.A.load('s', q, f'so_{self.centre}')
                                                           for q in range(self.Q)) + ';')

    def moments(self, L):
        """ρ, u (Guo: shifted by F/2 (/ρ)) and what the collision takes besides: u², u·F and 1 − ω/2 (Guo), the TRT
        rates a = (ω₊ + ω₋)/2, b = (ω₊ − ω₋)/2."""
        s, ct, D, Q, dirs = self.s, self.ct, self.D, self.Q, self.dirs
        L.append(f'  const {ct} rho = ' + ' + '.join(f'f{i}' for i in range(Q)) + ';')
        for a in range(D):
            pos = [f'f{i}' for i in range(Q) if dirs[i][a] == 1]
            neg = [f'f{i}' for i in range(Q) if dirs[i][a] == -1]
            L.append(f'  const {ct} m{a} = (' + ' + '.join(pos) + ') - (' + ' + '.join(neg) + ');')
        if s.compressible:
            L.append(f'  const {ct} irho = ({ct})1 / rho;')
        for a in range(D):
            half = f'({ct})0.5 * F{a}' if s.ff else self.c_(self.F[a] / 2) if s.fm == 'guo' else None
            m = f'(m{a} + {half})' if s.fm == 'guo' else f'm{a}'      # Guo: velocity shifted by F/2
            L.append(f'  const {ct} u{a} = {m}' + (' * irho;' if s.compressible else ';'))
        L.append(f'  const {ct} usq = ' + ' + '.join(f'u{a} * u{a}' for a in range(D)) + ';')
        self.smagorinsky_moments(L)
        if s.fm == 'guo':
            L.append(f'  const {ct} uF = ' + ' + '.join(f'u{a} * {self.Fa(a)}' for a in range(D)) + ';')
            L.append(f'  const {ct} kg = ({ct})1 - ({ct})0.5 * omega;')
        if s.trt is not None:
            if s.trt[0] == 'magic':
                lam = self.c_(s.trt[1])
                wo = f'(({ct})4 - ({ct})2 * omega) / (({ct})4 * {lam} * omega + ({ct})2 - omega)'
            else:
                wo = self.c_(s.trt[1])
            L.append(f'  const {ct} w_odd = {wo};')
            L.append(f'  const {ct} ta = ({ct})0.5 * (omega + w_odd), tb = ({ct})0.5 * (omega - w_odd);')

    # ---- the Smagorinsky subgrid model
    def smagorinsky_rate(self, L):
        """``lbm_omega_eff``, the one definition of the effective rate: ``ω_eff = 2 / (τ0 + R)``, ``τ0 = 1/ω0``,
        ``R = √(τ0² + 18 C_s² q)`` (R is returned too: the adjoint's chain factors read it)."""
        s, ct = self.s, self.ct
        if s.sm is None:
            return
        sqrt = '__builtin_sqrt' if ct == 'double' else '__builtin_sqrtf'
        L.append(f'{self.fn} {ct} lbm_omega_eff(const {ct} omega_0, const {ct} q, {ct}* R)\n{{')
        L.append(f'  const {ct} tau0 = ({ct})1 / omega_0;')
        L.append(f'  *R = {sqrt}(tau0 * tau0 + {self.c_(18 * s.sm * s.sm)} * q);')
        L.append(f'  return ({ct})2 / (tau0 + *R);\n}}')

    def smagorinsky_moments(self, L):
        """After ρ, u: ``Π_ab = Σ_i c_ia c_ib (f_i − feq_i)`` with the equilibrium's closed second moments
        ``ρ (δ_ab/3 + u_a u_b)`` (incompressible: ``ρ δ_ab/3 + u_a u_b``; exact for the second-order equilibrium on
        D2Q9, D3Q19 and D3Q27, whose weights are isotropic to fourth order), ``N = √(2 Σ_ab Π_ab²)`` over all D²
        entries, ``q = N/ρ`` (incompressible: ``N``) and ``omega``, the rate everything below reads."""
        s, ct, D = self.s, self.ct, self.D
        if s.sm is None:
            return
        sqrt = '__builtin_sqrt' if ct == 'double' else '__builtin_sqrtf'
        third = self.c_(1.0 / 3.0)
        for a in range(D):
            for b in range(a, D):
                pos = [f'f{i}' for i, c in enumerate(self.dirs) if c[a] * c[b] == 1]
                neg = [f'f{i}' for i, c in enumerate(self.dirs) if c[a] * c[b] == -1]
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
        L.append(f'  const {ct} omega = lbm_omega_eff({self.om0}, sm_q, &sm_R);')

    def sm_P(self, i):
        """``P_i = Σ_ab Π_ab c_ia c_ib`` of direction i (None for the rest direction, where it is 0)."""
        c = self.dirs[i]
        t = [f'sm_P{a}{a}' for a in range(self.D) if c[a]]
        t += [('- ' if c[a] * c[b] < 0 else '') + f'({self.ct})2 * sm_P{a}{b}'
              for a in range(self.D) for b in range(a + 1, self.D) if c[a] * c[b]]
        return '(' + ' + '.join(t).replace('+ - ', '- ') + ')' if t else None

    def smagorinsky_adjoint(self, L):
        """The chain factors of ``ω_eff(f, ω0)`` once ``dom = Σ_i g_i ∂dst_i/∂ω`` (at ω = ω_eff) is complete:

            v_k += dom ∂ω_eff/∂f_k,   ∂ω_eff/∂f_k = ∂ω_eff/∂q · ∂q/∂f_k,   ∂ω_eff/∂q = −ω_eff² K / (4R),  K = 18 C_s²
            ∂q/∂f_k = (∂N/∂f_k − q)/ρ  (incompressible: ∂N/∂f_k),   ∂N/∂f_k = (2/N)(P_k − Σ_i P_i ∂feq_i/∂f_k)

        With κ = dom ∂ω_eff/∂q and λ = 2κ/(Nρ) (incompressible: 2κ/N): ``v_k += λ P_k − Σ_i λ P_i ∂feq_i/∂f_k − κ q/ρ``
        (the last term compressible only). The middle sum has the form of the equilibrium sums of ``adjoint_sums``:
        they run over ``h_i − λ P_i`` — which is why ``dom`` is finished before them here, not after
        (``omega_adjoint``). Where N = 0, ∂N/∂f_k is defined as 0 (λ = 0): the reciprocal is guarded, no NaN.
        With an ω field: ``domega += dom ∂ω_eff/∂ω0``, ``∂ω_eff/∂ω0 = ω_eff² (1 + τ0/R) / (2 ω0²)``."""
        s, ct = self.s, self.ct
        if s.sm is None:
            return
        self.omega_adjoint_equilibria(L)
        K = self.c_(18 * s.sm * s.sm)
        L.append(f'  const {ct} sm_k = -dom * omega * omega * {K} / (({ct})4 * sm_R);')
        L.append(f'  const {ct} sm_iN = sm_N > ({ct})0 ? ({ct})1 / sm_N : ({ct})0;')
        L.append(f'  const {ct} sm_l = ({ct})2 * sm_k * sm_iN' + (' * irho;' if s.compressible else ';'))
        if s.compressible:
            L.append(f'  const {ct} sm_c = sm_k * sm_q * irho;')
        if s.of:
            L.append(f'  domega[wc] += (T)(dom * omega * omega * (({ct})1 + (({ct})1 / {self.om0}) / sm_R) / '
                     f'(({ct})2 * {self.om0} * {self.om0}));')

    def sm_fold(self, i, hi):
        """The weight of direction i in the equilibrium sums: ``h_i`` (``hi``), with Smagorinsky ``h_i − λ P_i``."""
        if self.s.sm is None or not self.sm_P(i):
            return hi
        return f'({hi} - sm_l * {self.sm_P(i)})'

    def obstacle_copy(self, L, p, off, sp, soff):
        """An obstacle cell keeps its state (forward: ``dst = src``; adjoint: ``out = g``): array ``sp`` at ``soff`` to
        array ``p`` at ``off`` (half floats: the bits themselves, no conversion on the way)."""
        A = self.A
        L.append(f'  const unsigned msk = nbmask[{self.cell}];')
        L.append(f'  if ((msk >> {SELF_BIT}) & 1u) {{')
        for i in range(self.Q):
            L.append('    ' + (A.copy(p, i, off, sp, soff) if self.s.h else A.store(p, i, off, A.load(sp, i, soff))))
        L.append('    return;\n  }')

    # ---- forward
    def forward_cell(self, L):
        """``lbm_fwd_cell``: pull (with the walls' links), collide, store.

        SRT: ``dst_i = f_i + ω (feq_i − f_i)``. TRT, with a = (ω₊ + ω₋)/2, b = (ω₊ − ω₋)/2: ``dst_i = (1 − a) f_i −
        b f_ī + a feq_i + b feq_ī``. MRT: ``dst = f − A (f − feq)``, ``A = ω P_ω + C``.
        Force: 'simple' adds the constant 3 w_i (c_i·F) to every fluid cell's post-collision value; 'guo' shifts the
        velocity by F/2 (/ρ) and adds w_i (1 − ω/2)(3 (c_i − u)·F + 9 (c_i·u)(c_i·F))."""
        s, A, ct, Q, w = self.s, self.A, self.ct, self.Q, self.w
        L.append(f'{self.fn} void lbm_fwd_cell({self.sig["fwd"]}, const int z, const int y, const int x)\n{{')
        L.append(f'  (void)Z; (void)s_bytes; (void)d_bytes; (void)wallid; {self.fstr_unused}')
        A.resource(L, 's')
        A.resource(L, 'd')
        _wrap_lines(L, self.axes)
        A.neighbour_offsets(L, 's')
        dcoff = A.cell_offset(L, 'd')
        if s.walls:
            self.obstacle_copy(L, 'd', dcoff, 's', f'so_{self.centre}')

        self.force_loads(L)
        self.omega_load(L)
        self.cell_density(L)
        self.pull_loads(L)
        self.moments(L)
        if s.trt is not None or s.mrt is not None:
            # TRT / MRT: every population's equilibrium first (the collision of i reads feq of other populations too)
            for i in range(Q):
                L.append(f'  {ct} fe{i};')
                self.cu_poly(L, i)
                L.append(f'    fe{i} = {self.feq(i)}; }}')
            if s.mrt is not None:
                L.append(f'  const {ct} ' + ', '.join(f'nq{k} = f{k} - fe{k}' for k in range(Q)) + ';')   # f − feq
        for i in range(Q):
            self.cu_poly(L, i)
            term = ''
            if s.fm == 'simple' and self.cFi(i):
                term = f' + {self.c_(3 * w[i])} * {self.cFi(i)}' if s.ff else f' + {self.c_(3 * w[i] * self.cF[i])}'
            elif s.fm == 'guo':
                term = (f' + {self.c_(w[i])} * kg * (({ct})3 * ({self.cFi(i) or self.c_(0)} - uF)'
                        + (f' + {self.cFi(i, 9)} * cu' if self.cFi(i) else '') + ')')
            if s.trt is not None:
                j = self.inv[i]
                val = (f'(({ct})1 - ta) * f{i} - tb * f{j} + ta * fe{i} + tb * fe{j}{term}' if j != i else
                       f'f{i} + omega * (fe{i} - f{i}){term}')
            elif s.mrt is not None:
                pw, cc = self.mat_row(s.mrt[0], 'nq', i), self.mat_row(s.mrt[1], 'nq', i)
                val = f'f{i}' + (f' - omega * ({pw})' if pw else '') + (f' - ({cc})' if cc else '') + term
            else:
                val = f'f{i} + omega * ({self.feq(i)} - f{i}){term}'
            L.append('    ' + A.store('d', i, dcoff, val + self.shift(i, ' - ')) + ' }')
        L.append('}')

    # ---- adjoint (scatter to where the forward pulled from)
    def adjoint_cell(self, L):
        """``lbm_adj_cell``: ``v_j = Σ_i g_i ∂dst_i/∂f_j`` of the cell's pulled pdfs through the collision's structure,
        each stored to where the forward pulled ``f_j`` from."""
        s, A, ct = self.s, self.A, self.ct
        L.append(f'{self.fn} void lbm_adj_cell({self.sig["adj"]}, const int z, const int y, const int x)\n{{')
        L.append(f'  (void)Z; (void)s_bytes; (void)g_bytes; (void)o_bytes; (void)wallid; {self.fstr_unused}')
        for p in 'sgo':
            A.resource(L, p)
        _wrap_lines(L, self.axes)
        A.neighbour_offsets(L, 's')
        A.neighbour_offsets(L, 'o')
        gcoff = A.cell_offset(L, 'g')
        if s.walls:
            self.prologue(L, gcoff)
        for i in range(self.Q):
            L.append(f'  const {ct} g{i} = {A.load("g", i, gcoff)};')
        self.force_loads(L)
        self.omega_load(L)
        self.cell_density(L)
        listed = s.fix and bool(s.gq_all)
        if listed:
            self.fix_loads(L)
        self.pull_loads(L, self.adj_progs, hoisted=listed and s.walls)
        self.moments(L)
        self.omega_adjoint_pdfs(L)
        self.smagorinsky_adjoint(L)
        if s.rho_links:
            L.append(f'  {ct} Rr = 0;')             # Σ_j βρ_j v_j over the cell's density-weighted links
        gown = s.g_own if s.fix else []
        if gown:
            L.append(f'  {ct} ' + ', '.join(f'G{q} = 0' for q in gown) + ';')      # Σ_j J_jq v_j (link programs)
        self.adjoint_sums(L)
        self.force_adjoint(L)
        self.omega_adjoint(L)
        if s.compressible:
            L.append(f'  const {ct} Bu = ' + ' + '.join(f'B{a} * u{a}' for a in range(self.D)) + ';')
        for j in range(self.Q):
            self.scatter(L, j)
        if s.rho_links:
            # the density term: slot Q of the scratch array with inline link programs, its only slot without
            L.append(f'  if (msk & {self.low}) rho_adj[{self.rho_slot()}{self.cell}] = Rr;')
        if gown:
            # out_q(x) += G_q: after the main launch's store of that entry, or (zeroed entry) in either order with this
            # launch's own atomic store into it — two addends onto zero, so the sum is the same either way
            L.append('  ' + ' '.join(A.atomic_add(A.lane('o', q, self.centre), f'G{q}') for q in gown))
        L.append('}')

    def rho_slot(self):
        return f'(IDX){self.Q} * {self.ncells} + ' if self.s.inl else ''

    def prologue(self, L, gcoff):
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
        s, A = self.s, self.A
        self.obstacle_copy(L, 'o', f'oo_{self.centre}', 'g', gcoff)
        if s.mode != 'main':
            return
        # a cell next to a program wall is the fix-up kernel's: it only zeroes the entries out_q(x), q in gq, that
        # the fix-up kernel adds its G_q into and whose writer also runs there (the cell itself when x + c_q is a
        # wall, or a listed neighbour x + c_q) — both contributions then arrive by atomic adds onto that zero
        L.append(f'  if ((msk >> {FIX_BIT}) & 1u) {{')
        for q in s.gq_all:
            zero = A.store('o', q, f'oo_{self.centre}', self.c_(0))
            if any(self.dirs[q]):
                iq = self.inv[q]
                kn = _key(self.dirs[iq])               # the neighbour x + c_q = x - c_(inv q)
                L.append(f'    if (((msk >> {iq}) & 1u) || ((nbmask[{self.ncell(kn)}] >> {FIX_BIT}) & 1u)) {zero}')
            else:
                L.append(f'    {zero}')
        L.append('    return;\n  }')

    def fix_loads(self, L):
        """The fix-up kernel: every listed cell has a program link, so its own pdfs (read by the links' programs and
        their Jacobians) and the wall ids of all its neighbours are loaded once, up front, beside the mask — no load
        of the kernel's latency-bound chain waits on the mask or on an id."""
        s = self.s
        used = sorted({int(m) for pg in s.programs if pg is not None for row in pg if row is not None
                       for m in re.findall(r'\bc(\d+)\b', ' '.join(row[0]) + ' ' + row[1] + ' ' +
                                           ' '.join(' '.join(r[1]) + ' ' + r[2] for r in row[2]))})
        if used:
            L.append('  ' + ' '.join(f'const {self.ct} c{q} = {self.A.load("s", q, f"so_{self.centre}")};'
                                     for q in used))
        if s.walls:
            L.append('  ' + ' '.join(f'const unsigned char wid{i} = wallid[{self.ncell(_key(self.dirs[i]))}];'
                                     for i in range(self.Q) if any(self.dirs[i])))

    def adjoint_sums(self, L):
        """The moment-like sums of the adjoint in scatter form (``_method.create_lb_adjoint_rule``):
        ``v_j = (1 − ω) g_j + ω (A + Σ_a B_a ∂u_a/∂f_j)`` with S = Σ_i g_i w_i, A = Σ_i g_i w_i (1 + poly_i) and
        B_a = Σ_i g_i w_i (3 + 9 c_i·u) c_ia (− 3 u_a S, in ``force_adjoint``).
        TRT takes them over h_i = a g_i + b g_ī: ``v_j = (1 − a) g_j − b g_ĵ + A_h + Σ_a B_h,a ∂u_a/∂f_j``; MRT over
        h = Aᵀ g: ``v_j = g_j − h_j + A_h + Σ_a B_h,a ∂u_a/∂f_j``."""
        s, ct, D, w = self.s, self.ct, self.D, self.w
        if s.mrt is not None:
            # h = Aᵀ g
            for i in range(self.Q):
                pw, cc = self.mat_row(s.mrt[0], 'g', i, True), self.mat_row(s.mrt[1], 'g', i, True)
                hv = ' + '.join(t for t in ((f'omega * ({pw})' if pw else None), (f'({cc})' if cc else None)) if t)
                L.append(f'  const {ct} h{i} = {hv or self.c_(0)};')
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
        for i in range(self.Q):
            self.cu_poly(L, i, poly=False)
            if s.trt is not None:
                # the equilibrium sums over h_i = a g_i + b g_ī (rest population: ω g_0)
                hi = f'(ta * g{i} + tb * g{self.inv[i]})' if self.inv[i] != i else f'omega * g{i}'
            else:
                # (Smagorinsky, SRT: h_i = ω g_i — the scatter then has no ω in front of the equilibrium part)
                hi = f'h{i}' if s.mrt is not None else f'omega * g{i}' if s.sm is not None else f'g{i}'
            hi = self.sm_fold(i, hi)
            L.append(f'    const {ct} gw = {hi} * {self.c_(w[i])};')
            L.append('    S += gw;')
            if s.gsplit:
                L.append(f'    const {ct} gwg = g{i} * {self.c_(w[i])};')
                L.append('    Sg += gwg;')
            if s.compressible:
                L.append(f'    A += gw * (({ct})1 + cu * (({ct})3 + ({ct})4.5 * cu) - ({ct})1.5 * usq);')
            if any(self.dirs[i]):
                L.append(f'    const {ct} t = gw * (({ct})3 + ({ct})9 * cu);')
                self.axis_sums(L, i, 'B', 't')
                if s.gsplit:
                    L.append(f'    const {ct} tg = gwg * (({ct})3 + ({ct})9 * cu);')
                    self.axis_sums(L, i, 'Bg', 'tg')
                if s.fm == 'guo' and self.cFi(i):
                    L.append(f'    const {ct} tf = {"gwg" if s.gsplit else "gw"} * {self.cFi(i)};')
                    self.axis_sums(L, i, 'E', 'tf')
                if s.ff and s.fm == 'simple':
                    self.axis_sums(L, i, 'M', f'(g{i} * {self.c_(w[i])})' if s.trt is not None or s.mrt is not None
                                   else 'gw')
            L.append('  }')
        if not s.compressible:
            L.append('  A = S;')

    def force_adjoint(self, L):
        """The velocity sensitivities B_a finished, with the force's part in them, and the force field's adjoint.

        'simple' leaves the adjoint unchanged. 'guo': the force term's derivative through u joins the velocity
        sensitivities: B_a += C_a / ω with C_a = (1 − ω/2) Σ_i g_i w_i (9 c_ia (c_i·F) − 3 F_a).
        ``force_field``: the adjoint ACCUMULATES the force adjoint into ``dforce`` (the strides of ``force``; every cell
        by one thread, so the T steps of the time-step op sum into one zeroed array): 'simple' ``dF_a = 3 Σ_i g_i w_i
        c_ia``; 'guo' — through the explicit term and the velocity shift ``∂u_a/∂F_a = 1/2 (/ρ)`` — ``dF_a = (1 − ω/2)
        Bf_a + ω B_a / 2 (/ρ)`` with ``Bf_a`` the equilibrium part of the velocity sensitivity (before the ρ scaling)
        and ``B_a`` the full one."""
        s, ct = self.s, self.ct
        for a in range(self.D):
            L.append(f'  B{a} -= ({ct})3 * u{a} * S;')
            if s.ff and s.fm == 'guo':
                # the explicit force term's F-derivative sums (over g: Bg for TRT / MRT, = B before the ρ scaling for
                # SRT)
                L.append(f'  const {ct} Bf{a} = ' + (f'Bg{a} - ({ct})3 * u{a} * Sg;' if s.gsplit else f'B{a};'))
            if s.compressible:
                L.append(f'  B{a} *= rho;')
            if s.gsplit:
                # the force term's derivative through u (TRT / MRT: v = g − h + A_h + Σ B_a ∂u_a/∂f_j, no ω factor)
                L.append(f'  B{a} += kg * (({ct})9 * E{a} - ({ct})3 * {self.Fa(a)} * Sg);')
            elif s.fm == 'guo':
                # the force term's derivative through u, scaled into B (v = … + ω (A + Σ B_a ∂u_a/∂f_j))
                L.append(f'  B{a} += kg * (({ct})9 * E{a} - ({ct})3 * {self.Fa(a)} * S) / omega;')
        if not s.ff:
            return
        # the force adjoint of this cell, accumulated over the op's steps
        for a in range(self.D):
            if s.fm == 'simple':
                val = f'({ct})3 * M{a}'
            else:
                # through the explicit term, and through the velocity shift ∂u_a/∂F_a = 1/2 (/ρ): Σ_i g_i ∂dst_i/∂u_a,
                # which is ω B_a for SRT (B carries 1/ω) and B_a for TRT / MRT
                sc = '' if s.gsplit else 'omega * '
                val = f'kg * Bf{a} + ({ct})0.5 * {sc}B{a}' + (' * irho' if s.compressible else '')
            L.append(f'  dforce[(IDX){a} * f_c + fc] += {val};')

    def omega_weight(self, k):
        """``q_k`` of ``dω = −Σ_k q_k n_k`` (``omega_adjoint``; None where it is the constant 0)."""
        s = self.s
        if s.trt is not None and self.inv[k] != k:
            return f'(tap * g{k} + tbp * g{self.inv[k]})'
        if s.mrt is not None:
            pw = self.mat_row(s.mrt[0], 'g', k, True)
            return f'({pw})' if pw else None
        return f'g{k}'

    def omega_adjoint_pdfs(self, L):
        """``omega_field``: the part of ``dω`` that reads the pulled pdfs, ``dom = −Σ_k q_k f_k`` — taken right after
        the moments, so that no ``f_k`` stays live through the adjoint's sums (``omega_adjoint`` has the formulas)."""
        s, ct = self.s, self.ct
        if not s.of and s.sm is None:
            return
        if s.trt is not None:
            if s.trt[0] == 'magic':
                lam = self.c_(s.trt[1])
                L.append(f'  const {ct} wden = ({ct})4 * {lam} * omega + ({ct})2 - omega;')
                L.append(f'  const {ct} wodp = -({ct})16 * {lam} / (wden * wden);')
            else:
                L.append(f'  const {ct} wodp = 0;')
            L.append(f'  const {ct} tap = ({ct})0.5 * (({ct})1 + wodp), tbp = ({ct})0.5 * (({ct})1 - wodp);')
        L.append(f'  {ct} dom = 0;')
        for k in range(self.Q):
            if self.omega_weight(k):
                L.append(f'  dom -= {self.omega_weight(k)} * f{k};')

    def omega_adjoint(self, L):
        """``omega_field``: the cell's ``dω(x) = Σ_i g_i ∂dst_i/∂ω``, ACCUMULATED into ``domega`` (the strides of the ω
        field; every cell by one thread of one adjoint launch per step — a listed cell by the fix-up launch, which
        the main launch's prologue left it to — so the T steps sum into one zeroed array without atomics).
        With ``n = f − feq``: ``dω = −Σ_k q_k n_k = −Σ_k q_k f_k`` (``omega_adjoint_pdfs``) ``+ Σ_k q_k feq_k`` (here:
        the equilibria recomputed from ρ, u — no load, and no pdf held in a register for it), a cancelling sum.

        SRT ``q = g``: ``dω = −Σ_i g_i n_i``. TRT ``dst_i = f_i − a n_i − b n_ī``: ``q_k = a′ g_k + b′ g_k̄``, ``a′ =
        (1 + ω₋′)/2``, ``b′ = (1 − ω₋′)/2``, ``ω₋′ = −16Λ / (4Λω + 2 − ω)²`` (magic number) or 0 (a constant odd rate);
        the rest population ``q_0 = g_0``. MRT ``dst = f − (ω P_ω + C) n``: ``q = P_ωᵀ g``. Guo's term
        ``w_i (1 − ω/2) T_i``, ``T_i = 3 (c_i − u)·F + 9 (c_i·u)(c_i·F)``, adds ``−½ Σ_i g_i w_i T_i``."""
        s = self.s
        if not s.of or s.sm is not None:
            return                                  # (Smagorinsky: ``smagorinsky_adjoint`` has stored it already)
        self.omega_adjoint_equilibria(L)
        L.append('  domega[wc] += (T)dom;')

    def omega_adjoint_equilibria(self, L):
        """``dom += Σ_k q_k feq_k`` and Guo's ``−½ Σ_i g_i w_i T_i`` (``omega_adjoint``)."""
        s, ct, w = self.s, self.ct, self.w
        if s.fm == 'guo':
            L.append(f'  {ct} domF = 0;')                 # Σ_i g_i w_i T_i
        for i in range(self.Q):
            self.cu_poly(L, i)
            if self.omega_weight(i):
                L.append(f'    dom += {self.omega_weight(i)} * ({self.feq(i)});')
            if s.fm == 'guo':
                L.append(f'    domF += g{i} * {self.c_(w[i])} * (({ct})3 * ({self.cFi(i) or self.c_(0)} - uF)'
                         + (f' + {self.cFi(i, 9)} * cu' if self.cFi(i) else '') + ');')
            L.append('  }')
        if s.fm == 'guo':
            L.append(f'  dom -= ({ct})0.5 * domF;')

    def scatter(self, L, j):
        """``v_j``, stored to the cell the forward pulled ``f_j`` from — ``(x − c_j, j)``, or ``(x, ī)`` for a bounced
        ``f_j`` (scaled by the link's γ). Without link programs every (component, cell) of the result is written
        exactly once (for fluid ``x``: by ``x + c_k`` if that cell is fluid, else by ``x`` itself; obstacle cells by
        themselves), so the output needs no zero fill and no atomics."""
        s, ct, Q, inv = self.s, self.ct, self.Q, self.inv
        cbs = self.signed_sum(j, 'B', paren=False) or f'({ct})0'
        du = f'(({cbs}) - Bu) * irho' if s.compressible else f'({cbs})'
        linked = s.walls and any(self.dirs[j]) and s.links is not None
        vq = '' if linked else 'const '
        # Smagorinsky: + dom ∂ω_eff/∂f_j beside the folded sums (``smagorinsky_adjoint``)
        sm = '' if s.sm is None else (f' + sm_l * {self.sm_P(j)}' if self.sm_P(j) else '') + \
            (' - sm_c' if s.compressible else '')
        if s.trt is not None and inv[j] != j:
            L.append(f'  {{ {vq}{ct} v = (({ct})1 - ta) * g{j} - tb * g{inv[j]} + (A + {du}){sm};')
        elif s.trt is not None:
            L.append(f'  {{ {vq}{ct} v = (({ct})1 - omega) * g{j} + (A + {du}){sm};')
        elif s.mrt is not None:
            L.append(f'  {{ {vq}{ct} v = g{j} - h{j} + (A + {du}){sm};')
        elif s.sm is not None:
            L.append(f'  {{ {vq}{ct} v = (({ct})1 - omega) * g{j} + (A + {du}){sm};')
        else:
            L.append(f'  {{ {vq}{ct} v = (({ct})1 - omega) * g{j} + omega * (A + {du});')
        taken = ''                  # (fix-up kernel) guard of the scatter store: not where a neighbour link is taken
        if linked:
            if s.rho_links:
                L.append(f'    if ((msk >> {j}) & 1u) Rr += lk_gr[id{j} * {Q} + {j}] * v;')
            cases = self.program_cases(j) if self.adj_progs else []
            if cases:
                taken = (self.scatter_programs_fix if s.fix else self.scatter_programs_inline)(L, j, cases)
            L.append(f'    if ((msk >> {j}) & 1u) v *= lk_g[id{j} * {Q} + {j}];')
        self.scatter_store(L, j, taken)

    def scatter_programs_fix(self, L, j, cases):
        """(Fix-up kernel) a program-linked component: Σ_j J_jq(c) v_j (c: the cell's own pre-streaming pdfs) into the
        G accumulators. A neighbour link (a program row of four, ``(lines, value, jac, offsets)``, Jacobian entries
        ``(k, lines_k, J, o)``) may read ``src_k(x + c_o)``. It is taken where every cell ``x + c_o`` it reads is fluid:
        bit ī_o of the cell's OWN mask word says so (it is the neighbour's ``SELF_BIT``, already in a register); it
        is the bounce-back otherwise: the wall id's table row is (α, β, γ) = (1, 0, 1), so the fused path has made
        ``f_j = src_ī(x)`` before the link's ``case`` and scatters ``v_j`` to ``(x, ī_j)`` after it. A taken link
        replaces both: the forward overwrites ``f_j``; the adjoint adds ``J·v_j`` into ``out_k(x + c_o)`` and drops the
        scatter to ``(x, ī_j)`` (the store is skipped: returns its guard)."""
        A = self.A
        taken = ''
        if any(len(pg) > 3 for _, pg in cases):
            L.append('    int tk = 0;')
            taken = 'if (!tk) { '
        L.append(f'    if ((msk >> {j}) & 1u) switch (id{j}) {{')
        for wid, pg in cases:
            if len(pg) > 3:
                # a neighbour link, where every cell it reads is fluid: J·v into the cells it read (atomic
                # adds: those entries are zeroed or stored by the main launch), and no bounce-back store
                # (``tk``: the zeroed entry of direction ī_j stays as it is)
                rows = ' '.join('{ ' + ' '.join(r[1]) + ' ' +
                                (A.atomic_add(A.lane('o', r[0], self.okey(r[3])), f'(T)(({r[2]}) * v)') if r[3] else
                                 f'G{r[0]} += ({r[2]}) * v;') + ' }' for r in pg[2])
                nl = self.nb_loads(rows, lambda q, kk: A.load('s', q, f'so_{kk}'))
                L.append(f'      case {wid}: if (!(msk & {self.omask(pg)})) {{ {nl} {rows} tk = 1; }} break;')
                continue
            if len({jl for _, jl, _ in pg[2]}) == 1:
                # one set of temporaries for the whole row (FixedDensity.program): emitted once
                rows = ' '.join(pg[2][0][1]) + ' ' + ' '.join(f'G{q} += ({je}) * v;' for q, _, je in pg[2])
            else:
                rows = ' '.join('{ ' + ' '.join(jl) + f' G{q} += ({je}) * v; }}' for q, jl, je in pg[2])
            L.append(f'      case {wid}: {{ {rows} }} break;')
        L.append('      default: break;\n    }')
        return taken

    def scatter_programs_inline(self, L, j, cases):
        """(C target) a program-linked component: its v for the second pass (the Jacobian row is evaluated there). The
        first pass writes every entry once, so where a neighbour link is taken it stores a zero to the bounce-back's
        entry ``(x, ī_j)``."""
        slot = f'rho_adj[(IDX){j} * {self.ncells} + {self.cell}]'
        L.append(f'    if ((msk >> {j}) & 1u) switch (id{j}) {{')
        own = [wid for wid, pg in cases if len(pg) < 4]
        if own:
            L.append('      ' + ' '.join(f'case {wid}:' for wid in own) + f' {slot} = v; break;')
        for wid, pg in cases:
            if len(pg) > 3:
                # a neighbour link where it is taken: v for the second pass, a zero for the bounce-back's entry
                L.append(f'      case {wid}: if (!(msk & {self.omask(pg)})) {{ {slot} = v; v = 0; }} break;')
        L.append('      default: break;\n    }')
        return ''

    def scatter_store(self, L, j, taken):
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
        s, A, inv = self.s, self.A, self.inv
        k = _key(self.dirs[j])
        gq = s.gq_all if s.fix else []
        walled = s.walls and any(self.dirs[j])
        bounced, pulled = A.lane('o', inv[j], self.centre), A.lane('o', j, k)
        if walled and (j in gq or inv[j] in gq):
            # a store into a G entry (component q in gq of a listed cell) is an atomic add onto the entry the main
            # kernel zeroed: the cell itself (bounced, component ī) or a listed neighbour x − c_j (component j)
            ab = 'true' if inv[j] in gq else 'false'
            an = f'((nbmask[{self.ncell(k)}] >> {FIX_BIT}) & 1u)' if j in gq else 'false'
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

    # ---- the adjoint's second pass
    def rho_cell(self, L):
        """``lbm_adj_rho_cell``: the density term of the cell's links reaches every component of the cell, whose adjoint
        entries the first pass wrote from other threads; with inline link programs (the C target) also ``Σ_j J_jk(c)
        v_j`` into component k of the cell, and a taken neighbour link's ``J·v`` into ``out_k(x + c_o)`` (``rho_adj``
        holds ``v_j``). That writes OTHER cells from other OpenMP threads: with neighbour links every update of this
        pass is an ``omp atomic`` one."""
        s, ct, Q = self.s, self.ct, self.Q
        L.append(f'{self.fn} void lbm_adj_rho_cell({self.sig["adj_rho"]}, const int z, const int y, const int x)\n{{')
        L.append('  (void)Z;')
        L.append(f'  const unsigned msk = nbmask[{self.cell}];')
        L.append(f'  if (((msk >> {SELF_BIT}) & 1u) || !(msk & {self.low})) return;')
        L.append(_cell_offset('o', self.axes))
        at = '_Pragma("omp atomic") ' if s.nb and not s.hip else ''
        if s.rho_links:
            L.append(f'  const {ct} R = rho_adj[{self.rho_slot()}{self.cell}];')
            for q in range(Q):
                L.append(f'  {at}out[(IDX){q} * o_q + oc] += R;')
        if not s.inl:
            L.append('}')
            return
        # Σ_j J_jk(c) v_j over the cell's program-linked components (c: the cell's own pre-streaming pdfs)
        _wrap_lines(L, self.axes)
        L.append(_cell_offset('s', self.axes))
        if s.nb:
            self.A.neighbour_offsets(L, 's')
            self.A.neighbour_offsets(L, 'o')

        def own(q):
            return f'({ct})src[(IDX){q} * s_q + sc]'
        for j in range(Q):
            cases = self.program_cases(j)
            if not cases:
                continue
            L.append(f'  if ((msk >> {j}) & 1u) {{')
            L.append(f'    const {ct} v = rho_adj[(IDX){j} * {self.ncells} + {self.cell}];')
            L.append(f'    switch (wallid[{self.ncell(_key(self.dirs[j]))}]) {{')
            for wid, pg in cases:
                if len(pg) > 3:
                    # a neighbour link, where it is taken: J·v into out_k(x + c_o)
                    rows = ' '.join('{ ' + ' '.join(r[1]) + f' {at}out[(IDX){r[0]} * o_q + ' +
                                    (f'oo_{self.okey(r[3])}' if r[3] else 'oc') + f'] += ({r[2]}) * v; }}'
                                    for r in pg[2])
                    nl = self.nb_loads(rows, lambda q, kk: f'({ct})src[(IDX){q} * s_q + so_{kk}]')
                    L.append(f'      case {wid}: if (!(msk & {self.omask(pg)})) {{ {self.own_loads(rows, own)} {nl} '
                             f'{rows} }} break;')
                    continue
                rows = ' '.join('{ ' + ' '.join(jl) + f' {at}out[(IDX){q} * o_q + oc] += ({je}) * v; }}'
                                for q, jl, je in pg[2])
                L.append(f'      case {wid}: {{ {self.own_loads(rows, own)} {rows} }} break;')
            L.append('      default: break;\n    }\n  }')
        L.append('}')

    # ---- entry points
    def hip_fix_entry(self, L):
        """The fix-up kernel: one thread per listed cell (the fluid cells next to a link-program wall).
        One wave per workgroup (FIX_BLOCK lanes): the few listed cells spread over as many CUs as possible — each wave
        runs a long, branchy, latency-bound chain, and waves of one CU would share its scalar unit."""
        L.append(f'extern "C" __global__ void __launch_bounds__({FIX_BLOCK}) lbm_adj_fix({self.sig["adj"]}, '
                 'const int* __restrict__ cells, const int ncell)\n{')
        L.append(f'  const int t = (int)(blockIdx.x * {FIX_BLOCK}u + threadIdx.x);')
        L.append('  if (t >= ncell) return;')
        L.append('  const unsigned cell = (unsigned)cells[t];')
        L.append(CELL_ZYX)
        L.append(f'  lbm_adj_cell({self.args["adj"]}, z, y, x);\n}}')

    def hip_grid_entries(self, L):
        """``lbm_fwd``, ``lbm_adj`` (and ``lbm_adj_rho``): one thread per cell.
        A block = 256 consecutive cells of the lattice in C order (rows of x), and consecutive blocks on one XCD
        (bijective remap of the round-robin dispatch): a lattice row's x-shifted loads and the adjoint's
        x-shifted stores cover cache lines that the neighbouring wave also touches — in one block, or in a
        block on the same XCD's L2, not split between two L2s (partial-line write-backs)."""
        for k in ('fwd', 'adj') + (('adj_rho',) if self.s.two else ()):
            L.append(f'extern "C" __global__ void __launch_bounds__(256) lbm_{k}({self.sig[k]})\n{{')
            L.append('  const unsigned nb = gridDim.x, b = blockIdx.x;')
            L.append('  const unsigned per = nb >> 3, rem = nb & 7, xcd = b & 7, bi = b >> 3;')
            L.append('  const unsigned lb = (xcd < rem) ? xcd * (per + 1) + bi : rem * (per + 1) + (xcd - rem) * per + bi;')
            L.append('  const unsigned cell = lb * 256u + threadIdx.x;     // cells < 2^32 (checked at launch)')
            L.append('  if (cell >= (unsigned)X * (unsigned)Y * (unsigned)Z) return;')
            L.append(CELL_ZYX)
            L.append(f'  lbm_{k}_cell({self.args[k]}, z, y, x);\n}}')

    def c_entries(self, L):
        """The C loop nests, with the CPU kernels' ctypes signature (``backends.cpu_kernel.compile_c``): pointers,
        extents, strides, -, scalars. ``lbm_adj`` runs the second pass after every cell's scatter, in the same call."""
        s, ct = self.s, self.ct
        for k, pdfs in (('fwd', 'sd'), ('adj', 'sgo')):
            adj, n = k == 'adj', len(pdfs)
            L.append(f'void lbm_{k}(void** P, const i64* N, const i64* S, const i64* B_, const double* Dv)\n{{')
            L.append('  (void)B_; const int Z = (int)N[0], Y = (int)N[1], X = (int)N[2];')
            L.append(f'  const {ct} {self.om_arg} = ({ct})Dv[0];')
            ptrs = [('const T*', ARRAYS[p]) for p in pdfs[:-1]] + [('T*', ARRAYS[pdfs[-1]])] + \
                [('const unsigned*', 'nbmask'), ('const unsigned char*', 'wallid')]
            L.append('  ' + ' '.join(f'{ty} {nm} = ({ty})P[{i}];' for i, (ty, nm) in enumerate(ptrs)))
            L.append('  const IDX ' + ', '.join(f'{p}_{a} = S[{4 * i + j}]' for i, p in enumerate(pdfs)
                                                for j, a in enumerate('qzyx')) + ';')
            if s.ff:
                L.append(f'  const T* force = (const T*)P[{n + 2}];' + (f' T* dforce = (T*)P[{n + 3}];' if adj else ''))
                L.append('  const IDX ' + ', '.join(f'f_{a} = S[{4 * n + j}]' for j, a in enumerate('czyx')) + ';')
            nf = n + 2 + ((2 if adj else 1) if s.ff else 0)       # pointers before the ω field's
            if s.of:
                L.append(f'  const T* omf = (const T*)P[{nf}];' + (f' T* domega = (T*)P[{nf + 1}];' if adj else ''))
                L.append('  const IDX ' + ', '.join(f'w_{a} = S[{4 * n + (4 if s.ff else 0) + j}]'
                                                    for j, a in enumerate('zyx')) + ';')
            if adj and s.two:
                L.append(f'  T* rho_adj = (T*)P[{n + (4 if s.ff else 2) + (2 if s.of else 0)}];')
            L.append('  const long long ' + ', '.join(f'{p}_bytes = 0' for p in pdfs) + ';')
            for cellfn in (k, 'adj_rho') if adj and s.two else (k,):
                # (the density pass after every cell's scatter: the C target runs both passes in one call)
                L.append(C_LOOPS)
                L.append(f'        lbm_{cellfn}_cell({self.args[cellfn]}, z, y, x);')
            L.append('}')
