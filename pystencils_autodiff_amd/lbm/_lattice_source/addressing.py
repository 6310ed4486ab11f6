"""How the lattice kernels reach the pdf arrays: buffer resources or plain pointers, loads, stores and copies."""
from .spec import ARRAYS


class Addressing:
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
        L.append(cell_offset(p, self.axes))
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


def cell_offset(p, axes):
    return f'  const IDX {p}c = ' + ' + '.join(f'(IDX){a} * {p}_{a}' for a in axes) + ';'


def wrap_lines(L, axes):
    """The periodic neighbours' coordinates."""
    for a in axes:
        N = a.upper()
        L.append(f'  const int {a}m = {a} == 0 ? {N} - 1 : {a} - 1, {a}p = {a} == {N} - 1 ? 0 : {a} + 1;')
