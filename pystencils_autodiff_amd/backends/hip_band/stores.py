"""The stores of one output plane: a lane's rows as 16-byte chunks, whole, masked by row or masked by cell."""


def _st128(val, off):
    return f'__builtin_amdgcn_raw_buffer_store_b128({val}, ors, {off}, 0, 2);'


def _tail_parts(T):
    """A row's partial last chunk as (whole dwords, then halves: one when X is odd)."""
    nb = (T.X % T.VE) * T.es
    return nb // 4, (nb % 4) // 2


def tail_store(T, vec, base, k=None):
    """The partial last chunk of vector ``vec`` at offset ``base`` (+ ``k`` bytes): whole dwords, then the odd
    element's half."""
    ndw, nh = _tail_parts(T)
    out, c = [], 'xyzw'
    if ndw:
        ty = {1: 'unsigned', 2: 'u32x2', 3: 'u32x3'}[ndw]
        out.append(f'__builtin_amdgcn_raw_buffer_store_b{32 * ndw}(({ty}){vec}.{c[:ndw]}, ors, '
                   f'{base if k is None else f"{base} + {k}u"}, 0, 2);')
    if nh:
        out.append(f'__builtin_amdgcn_raw_buffer_store_b16((unsigned short){vec}.{c[ndw]}, ors, '
                   f'{base} + {(k or 0) + 4 * ndw}u, 0, 2);')
    return out


def tail_load(T, dst, k):
    """Read the current contents of the partial last chunk (``k`` bytes past ``sofs``) into ``dst``
    (read-modify-write)."""
    ndw, nh = _tail_parts(T)
    out, c = [], 'xyzw'
    if ndw == 1:
        out.append(f'{dst}.x = __builtin_amdgcn_raw_buffer_load_b32(ors, sofs + {k}u, 0, 0);')
    elif ndw:
        ty = {2: 'u32x2', 3: 'u32x3'}[ndw]
        out.append(f'{{ const {ty} t = __builtin_amdgcn_raw_buffer_load_b{32 * ndw}(ors, '
                   f'sofs + {k}u, 0, 0); ' + ' '.join(f'{dst}.{c[i]} = t.{c[i]};' for i in range(ndw)) + ' }')
    if nh:
        out.append(f'{dst}.{c[ndw]} = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(ors, '
                   f'sofs + {k + 4 * ndw}u, 0, 0);')
    return ' '.join(out)


def tail_shift_lines(T, src, dst):
    """``dst`` = the 16 bytes ending at the row's end: the left lane's last ``tail_sb`` bytes, then ``src``'s
    first 16 - tail_sb bytes (dword selects, and v_alignbyte when the shift is not whole dwords)."""
    q, b = T.tail_sb // 4, T.tail_sb % 4
    k0 = 4 - q - (1 if b else 0)                      # first dword of the result in (left lane | own)
    need = sorted({k0 + i for i in range(4)} | ({k0 + i + 1 for i in range(4)} if b else set()))
    out = []
    seq = {}
    for k in need:
        if k < 4:                                     # the left lane's dword k (wave_shr:1)
            out.append(f'const unsigned nb{k} = __builtin_amdgcn_update_dpp(0u, {src}.{"xyzw"[k]}, 0x138, 0xf, 0xf, '
                       'false);')
            seq[k] = f'nb{k}'
        else:
            seq[k] = f'{src}.{"xyzw"[k - 4]}'
    if b:
        parts = [f'__builtin_amdgcn_alignbyte({seq[k0 + i + 1]}, {seq[k0 + i]}, {4 - b}u)' for i in range(4)]
    else:
        parts = [seq[k0 + i] for i in range(4)]
    out.append(f'const u32x4 {dst} = {{{", ".join(parts)}}};')
    return out


def _row_whole(T, ind, k, bit, ov):
    """A row of whole-row stores (``BXW``): no branches. A row outside [ylo, yhi) (or an idle lane's) stores at an
    offset past the buffer's range, which the range check drops; a partial last chunk stores its whole dwords (and
    half) at the row offset while its 16-byte store is dropped, every other lane the reverse."""
    B = [f'{ind}  {{ {ov} const unsigned ro = ((rowok & {bit}u) ? sofs + {k}u : 0x7ffffff0u);']
    if T.partial:
        B.append(f'{ind}    const u32x4 ow = __builtin_bit_cast(u32x4, ov);')
    if T.tail_shift:
        # the row's partial last chunk as ONE 16-byte store of the row's last VE cells, shifted left by
        # the sb bytes the chunk lacks: the first of them are the left lane's last cells (DPP wave_shr:1,
        # the same row; that lane stores the same values there), so the row takes one store instruction
        # instead of three (16-byte, then dword and half stores that drop 63 lanes each)
        B += [f'{ind}    {ln}' for ln in tail_shift_lines(T, 'ow', 'tw')]
        B.append(f'{ind}    ' + _st128('xtail ? tw : ow', f'xtail ? ro - {T.tail_sb}u : ro'))
    elif T.partial:
        B.append(f'{ind}    ' + _st128('ow', 'xtail ? 0x7ffffff0u : ro'))
        # (the tail store under a branch on the tail lanes measured slower: profiles/r05_pitch_btb.log)
        B.append(f'{ind}    const unsigned rt = xtail ? ro : 0x7ffffff0u;')
        B += [f'{ind}    {t}' for t in tail_store(T, 'ow', 'rt')]
    else:
        B.append(f'{ind}    ' + _st128('__builtin_bit_cast(u32x4, ov)', 'ro'))
    return B + [f'{ind}  }}']


def _row_cells(T, ind, k, bit, ov, cells):
    """A row masked cell by cell: whole in-range chunks as they are; of the others the cells outside [xlo, xhi) are
    zeros (``XB``: the row is stored whole) or keep their contents (read-modify-write). 'bu' rows: the partial last
    chunk holds X % VE cells of the row (the rest is the next row's), stored as whole dwords and the odd half."""
    B = [f'{ind}  if (rowok & {bit}u) {{',
         f'{ind}    {ov}',
         f'{ind}    if (xfull) {{',
         f'{ind}      ' + _st128('__builtin_bit_cast(u32x4, ov)', f'sofs + {k}u'),
         f'{ind}    }} else {{']
    if T.cfg.XB:
        # x border cells: zeros; each cell selected on its own
        sel = ', '.join(f'(x + {q} >= xlo && x + {q} < xhi) ? {cells[q]} : ({T.et})0' for q in range(T.VE))
        B.append(f'{ind}      const {T.vt} zv = {{{sel}}};')
        full, vec = '__builtin_bit_cast(u32x4, zv)', 'zw'
        if T.partial:
            B.append(f'{ind}      const u32x4 zw = __builtin_bit_cast(u32x4, zv);')
    else:
        # read-modify-write of the lane's chunk (the whole chunk, or the partial last one), cells selected one by one
        # (per-cell stores cost ~30 VGPRs in the loop)
        B.append(f'{ind}      const u32x4 ow = __builtin_bit_cast(u32x4, ov);')
        B.append(f'{ind}      u32x4 old;')
        if T.partial:
            B.append(f'{ind}      if (xtail) {{ old = (u32x4)(0u); {tail_load(T, "old", k)} }}')
            B.append(f'{ind}      else old = __builtin_amdgcn_raw_buffer_load_b128(ors, sofs + {k}u, 0, 0);')
        else:
            B.append(f'{ind}      old = __builtin_amdgcn_raw_buffer_load_b128(ors, sofs + {k}u, 0, 0);')
        nw = []
        for d, c in enumerate('xyzw'):
            if T.half:
                lo = f'(x + {2 * d} >= xlo && x + {2 * d} < xhi)'
                hi = f'(x + {2 * d + 1} >= xlo && x + {2 * d + 1} < xhi)'
                nw.append(f'(({lo} ? ow.{c} : old.{c}) & 0xffffu) | (({hi} ? ow.{c} : old.{c}) & 0xffff0000u)')
            else:
                nw.append(f'(x + {d} >= xlo && x + {d} < xhi) ? ow.{c} : old.{c}')
        B.append(f'{ind}      const u32x4 nw = {{{", ".join(nw)}}};')
        full, vec = 'nw', 'nw'
    full = _st128(full, f'sofs + {k}u')
    if T.partial:
        B.append(f'{ind}      if (xtail) {{ {" ".join(tail_store(T, vec, "sofs", k))} }} else {{ {full} }}')
    else:
        B.append(f'{ind}      {full}')
    return B + [f'{ind}    }}', f'{ind}  }}']


def stores(T, ind, si, sp, fld):
    """Output plane ``zb - 2 + jj`` of field ``fld`` from accumulator set ``sp`` of plan ``si``."""
    B = [f'{ind}{{',
         f'{ind}  const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc('
         f'(void*)(f_{fld.name} + (i64)(zb - 2 + jj) * YX), (short)0, (int)(YX * {T.es}), 0x00020000);']
    for o in range(T.R):
        cells = [T.cell(si, sp, o, q) for q in range(T.VE)]
        ov = f'const {T.vt} ov = {{{", ".join(cells)}}};'
        k = o * T.X * T.es                               # byte offset of the lane's row o from its first
        if not T.cfg.BMASK:
            # every row of every band inside [ylo, yhi), x range = whole rows (checked at plan time)
            B.append(f'{ind}  {{ {ov} ' + _st128('__builtin_bit_cast(u32x4, ov)', f'sofs + {k}u') + ' }')
        elif T.cfg.BXW:
            B += _row_whole(T, ind, k, 1 << o, ov)
        else:
            B += _row_cells(T, ind, k, 1 << o, ov, cells)
    B.append(f'{ind}}}')
    if T.cfg.BNT != 2:
        # store cache policy probe (2 = non-temporal, the default)
        B = [ln.replace(', 0, 2);', f', 0, {T.cfg.BNT});') if 'raw_buffer_store' in ln else ln for ln in B]
    return B
