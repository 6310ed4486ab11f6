"""The ``zsum`` schedule over a half-precision LDS ring (fp16 storage, fp32 arithmetic)."""
from dataclasses import dataclass

import sympy as sp

from ..printer import KernelExprPrinter
from .common import PRELUDE, _tag, retirement_lines
from .loader import WS_CONSUMER_BARRIER, _ws_loader, ws_plane_base
from .prelude import _march_prelude


@dataclass
class HalfPlan:
    """What the half ring reads and accumulates per plane. ``chains[(si, dz, nr, q, c)]``: the fused multiply-add terms
    Σ coeff · (u[x+e], u[x+e+2]) of plan ``si``'s cell pair ``c`` of quad ``q`` in row ``nr``; ``rows``: the tap rows
    (field, jr); ``dwords[row]``: (the element offsets ``e`` whose pairs the chains name, the dwords covering
    x-RX .. x+CX-1+RX), both relative to the lane's first cell; ``groups``: the accumulator groups (si, nr, q, c)."""
    ir: object
    cfg: object
    plans: list
    g: dict
    ws: dict
    Q: int
    chains: dict
    rows: list
    dwords: dict
    groups: list

    def dpp_row(self, row):
        """The row's dwords are the lane's own and one on each side (from the neighbour lanes by DPP)."""
        return self.dwords[row][1] == list(range(-1, 2 * self.Q + 1))

    def terms(self, group, dz):
        si, nr, q, c = group
        parts = self.chains.get((si, dz, nr, q, c))
        return ' + '.join(f'({t})' for t in parts) if parts else None


def _pname(fname, jr, e0):
    return f"pp_{fname}_{_tag(jr)}_{_tag(e0)}"


def _acc(group, k):
    si, nr, q, c = group
    return f"a{si}_{k}_{nr}_{q}_{c}"


def _hname(st, fn, jr, d):
    return f'h{st}_{fn}_{_tag(jr)}_{_tag(d)}'


def half_plan(ir, cfg, plans, g, ws):
    """The ``HalfPlan`` of ``zsum_plan``'s ``plans``: the chains per (plan, dz, row, quad, parity) and, per tap row, the
    dwords that cover the elements they name. Planning only, no line is printed here."""
    Q = cfg.CX // 4
    chains, needed = {}, set()
    for si, pl in enumerate(plans):
        for dz, terms in pl['lin'].items():
            for nr in range(cfg.NR):
                for q in range(Q):
                    for c in (0, 1):
                        parts = []
                        for coeff, f, dy, dx, k in terms:
                            e0 = 4 * q + c + dx
                            needed.add((f.name, nr + dy, e0))
                            v = _pname(f.name, nr + dy, e0)
                            sym = sp.Symbol(v)
                            parts.append(KernelExprPrinter('float', {**ir.symbol_names, sym: v}).doprint_expr(coeff * sym))
                        chains[(si, dz, nr, q, c)] = parts
    rows = sorted({(fn, jr) for fn, jr, _ in needed})
    dwords = {}
    for fn, jr in rows:
        es = sorted(e for f_, j_, e in needed if (f_, j_) == (fn, jr))
        dwords[(fn, jr)] = (es, list(range(min(es) // 2, (max(es) + 2) // 2 + 1)))
    groups = [(si, nr, q, c) for si in range(len(plans)) for nr in range(cfg.NR) for q in range(Q) for c in (0, 1)]
    return HalfPlan(ir, cfg, plans, g, ws, Q, chains, rows, dwords, groups)


def _dpp_row_reads(ind, t, row, Q, own, neighbour, as_int, e2):
    """One tap row whose dwords are the lane's own and one on each side. Own dwords 0..2Q-1: 8-byte reads,
    conflict-free (64 banks per 32-lane group); dword -1 / 2Q from lane l-1 / l+1, the wave's end lanes from one
    ds_read_b32 whose other lanes read distinct banks (eoff_). ``own(d, value)`` / ``neighbour(d, value)`` print the
    line that finalises dword ``d``, ``as_int(d)`` names it as a DPP operand. ``e2``: rows on half dwords also take
    dword 2Q+1 — 1 = read after the edge dwords, 2 = read with them, 0 = not at all."""
    def dpp(e, src, ctl):
        return f'__builtin_amdgcn_update_dpp({e}, {src}, {ctl}, 0xf, 0xf, false)'
    R = []
    # (element accesses of a vector are not bit-cast directly: clang then casts element 0)
    for q2 in range(Q):
        R.append(f'{ind}const f16x4 o{t}_{q2} = *(const f16x4*)({row} + {4 * q2});')
        for c in (0, 1):
            R.append(own(2 * q2 + c, f'__builtin_shufflevector(o{t}_{q2}, o{t}_{q2}, {2 * c}, {2 * c + 1})'))
    R.append(f'{ind}const int e{t} = *(const int*)({row} + eoff_);')
    second = f'{ind}const int e2{t} = *(const int*)({row} + eoff_ + 2);'
    if e2 == 2:
        R.append(second)
    R.append(neighbour(-1, dpp(f'e{t}', as_int(2 * Q - 1), '0x138')))
    R.append(neighbour(2 * Q, dpp(f'e{t}', as_int(0), '0x130')))
    if e2 == 1:
        R.append(second)
    if e2:
        R.append(neighbour(2 * Q + 1, dpp(f'e2{t}', as_int(1), '0x130')))
    return R


def _row_reads_xo(H, ind, st, row, fn, jr, decl, sh):
    """A tap row of an XO kernel (rows on half dwords: the loader brought such a row one element early): the lane reads
    the aligned dwords as ints and realigns them (v_alignbit) where the row's first element sits on a half dword —
    ``sh`` = 0 / 1 where the code knows, ``None`` for a select on the row's ``sh<row>`` flag."""
    t = f'{st}_{fn}_{_tag(jr)}'
    Q = H.Q
    if H.dpp_row((fn, jr)):
        def raw(d):
            return f'r{t}_{"m1" if d < 0 else d}'
        R = _dpp_row_reads(ind, t, row, Q, lambda d, v: f'{ind}const int {raw(d)} = __builtin_bit_cast(int, {v});',
                           lambda d, v: f'{ind}const int {raw(d)} = {v};', raw, 2 if sh is None else sh)
        ds = range(-1, 2 * Q + 1)
    else:
        def raw(d):
            return f'r{t}_{_tag(d)}'
        ds = H.dwords[(fn, jr)][1]
        R = [f'{ind}const int {raw(d)} = *(const int*)({row} + {2 * d});'
             for d in range(ds[0], ds[-1] + 1 + (1 if sh is None else sh))]
    for d in ds:
        align = f'__builtin_amdgcn_alignbit((unsigned){raw(d + 1)}, (unsigned){raw(d)}, 16u)'
        value = raw(d) if sh == 0 else align if sh else f'sh{t} ? {align} : (unsigned){raw(d)}'
        R.append(f'{ind}{"const f16x2 " if decl else ""}{_hname(st, fn, jr, d)} = __builtin_bit_cast(f16x2, {value});')
    return R


def _reads(H, ind, st, slot_expr, decl, shmap=None):
    """Tap-row dwords of plane slot ``slot_expr`` into the ``h*`` names (``decl``: declare them). XO rows:
    ``shmap`` = {(field, jr): 0 / 1} — the rows that start on a half dword, known at this point of the code
    (the plane loop branches on the parity of the lane's first row) — else a per-row select."""
    cfg, FG, Q = H.cfg, H.g['FG'], H.Q
    R = []
    if cfg.XO and shmap is None:
        for f in H.ir.stencil_fields:
            R.append(f'{ind}const int pp_{f.name} = hpar({ws_plane_base(f, H.g["RZ"], "p")});')
    for fn, jr in H.rows:
        row = f'lds_{fn} + ({slot_expr}) * {H.ws["F"][fn]["SLOT"]} + lb_{fn} + {jr * FG[fn]["P"]}'
        if cfg.XO:
            if shmap is None:
                R.append(f'{ind}const bool sh{st}_{fn}_{_tag(jr)} = (((ybase + {jr}) * X * {FG[fn]["C"]} + pp_{fn}) & 1) '
                         '!= 0;')
            R += _row_reads_xo(H, ind, st, row, fn, jr, decl, shmap and shmap[(fn, jr)])
        elif H.dpp_row((fn, jr)):
            def h(d):
                return _hname(st, fn, jr, d)
            R += _dpp_row_reads(ind, f'{st}_{fn}_{_tag(jr)}', row, Q, lambda d, v: f'{ind}const f16x2 {h(d)} = {v};',
                                lambda d, v: f'{ind}const f16x2 {h(d)} = __builtin_bit_cast(f16x2, {v});',
                                lambda d: f'__builtin_bit_cast(int, {h(d)})', 0)
        else:
            R += [f'{ind}{"const f16x2 " if decl else ""}{_hname(st, fn, jr, d)} = *(const f16x2*)({row} + {2 * d});'
                  for d in H.dwords[(fn, jr)][1]]
    return R


def _stores(H, ind):
    """Stores of output plane p - RZ: quads (x, x+1, x+2, x+3) = (a_0.x, a_1.x, a_0.y, a_1.y)."""
    cfg, plans, RZ = H.cfg, H.plans, H.g['RZ']
    B = [f'{ind}if (p - {RZ} >= zb) {{', f'{ind}  const i64 ooff = (i64)(p - {RZ}) * YX;']
    for pl in plans:
        fo = pl['field'].name
        B.append(f'{ind}  const __amdgpu_buffer_rsrc_t orsrc_{fo} = __builtin_amdgcn_make_buffer_rsrc((void*)(f_{fo} + '
                 f'ooff), (short)0, (int)(YX * 2), 0x00020000);')
    for nr in range(cfg.NR):
        for q in range(H.Q):
            B.append(f'{ind}  {{')
            B.append(f'{ind}    const int y = ybase + {nr};')
            B.append(f'{ind}    const int x = xbase + {4 * q};')
            B.append(f'{ind}    if (y >= ylo && y < yhi) {{')
            for si, pl in enumerate(plans):
                a0, a1 = _acc((si, nr, q, 0), 0), _acc((si, nr, q, 1), 0)
                B.append(f'{ind}      f32x4 v{si} = {{{a0}.x, {a1}.x, {a0}.y, {a1}.y}};')
            if cfg.XB:
                B.append(f'{ind}      #pragma unroll')
                B.append(f'{ind}      for (int e = 0; e < 4; ++e) if (x + e < xlo || x + e >= xhi) '
                         + ' '.join(f'v{si}[e] = 0.0f;' for si in range(len(plans))))
                full, part = 'x + 3 < X', 'x + e < X'
            else:
                full, part = 'x >= xlo && x + 3 < xhi', 'x + e >= xlo && x + e < xhi'
            B.append(f'{ind}      if ({full}) {{')
            for si, pl in enumerate(plans):
                fo = pl['field'].name
                val = f'__builtin_convertvector(v{si}, f16x4)'
                # buffer store: the plane's descriptor (uniform) + the row's hoisted 32-bit byte offset,
                # no 64-bit address arithmetic per plane
                B.append(f'{ind}        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, {val}), '
                         f'orsrc_{fo}, rb_{nr}_{q}, 0, {2 if cfg.NT_STORE else 0});')
            B.append(f'{ind}      }} else {{')
            B.append(f'{ind}        #pragma unroll')
            B.append(f'{ind}        for (int e = 0; e < 4; ++e) if ({part}) {{')
            for si, pl in enumerate(plans):
                B.append(f'{ind}          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, '
                         f'(_Float16)v{si}[e]), orsrc_{pl["field"].name}, rb_{nr}_{q} + 2 * e, 0, 0);')
            B.append(f'{ind}        }}')
            B.append(f'{ind}      }}')
            B.append(f'{ind}    }}')
            B.append(f'{ind}  }}')
    B.append(f'{ind}}}')
    return B


def _compute(H, ind, st):
    """Plane p from the raw dwords of set ``st``: fp32 pairs, the dz = RZ chains into a_0, the store of
    output p - RZ, the retirement chains."""
    B = []
    for fn, jr in H.rows:
        for e0 in H.dwords[(fn, jr)][0]:
            def el(e):
                return f'{_hname(st, fn, jr, e // 2)}[{e % 2}]'
            B.append(f'{ind}const f32x2 {_pname(fn, jr, e0)} = {{(float){el(e0)}, (float){el(e0 + 2)}}};')
    # (a kernel without z radius has no accumulator slots: its one value per cell pair is declared where it is formed)
    before, after = retirement_lines(ind, H.g['RZ'], H.groups, lambda gr, k: _acc(gr, 0 if k == 't' else k), H.terms,
                                     '(f32x2)(0)', temp='const f32x2 ')
    return B + before + _stores(H, ind) + after


def _emit_zsum_half(ir, name, cfg, plans, g, ws):
    """zsum over a half-precision LDS ring (fp16 storage, fp32 arithmetic): the loader wave DMAs the raw
    fp16 plane images (``_ws_loader``), each compute lane owns ``CX`` x-ADJACENT cells of ``NR`` rows.

    Per plane and tap row a lane reads its cells' fp16 values and the ``RX`` neighbours on each side as
    dwords (one ``ds_read_b64`` for a quad plus the side dwords), converts each value once or twice into
    fp32 pairs ``(u[x+e], u[x+e+2])``, and runs ``v_pk_fma_f32`` chains over the cell pairs
    ``(x, x+2)`` / ``(x+1, x+3)`` of each quad into ``2·RZ`` accumulators (fused retirement, as
    ``emit_zsum``). Finished quads go out as one 8-byte non-temporal store (two ``v_cvt_pk_f16_f32``).
    Versus staging fp32 planes through registers: the compute waves issue no global load, so no
    ``s_waitcnt vmcnt(0)`` (which also waited for their own stores) and no LDS write per plane."""
    RZ, RY, RX, H_ = (g[k] for k in ('RZ', 'RY', 'RX', 'H'))
    stencil = ir.stencil_fields
    CX, NR = cfg.CX, cfg.NR
    S = 2 * RZ
    H = half_plan(ir, cfg, plans, g, ws)
    Q, rows = H.Q, H.rows
    L = [PRELUDE, 'typedef unsigned u32x2 __attribute__((ext_vector_type(2)));']
    L.append(f"// zsum schedule over a half-precision LDS ring: TX={cfg.TX} TY={cfg.TY} ({CX} x-adjacent cells x "
             f"{NR} rows per lane), LDS-DMA loader wave, {ws['NS']}-slot fp16 plane ring, {ws['D']} planes in flight, "
             f"{max(1, S)} register accumulators per cell and output, radius(z,y,x)=({RZ},{RY},{RX}), halo H={H_}, "
             f"pitch P={g['P']}, LDS {ws['lds_bytes']} B")
    L += _march_prelude(ir, name, cfg, g, {f.name: 1 for f in stencil}, ws=ws, lane_stride=CX)
    if cfg.XO:
        L.append('  auto hpar = [&](const void* b) { return b ? (int)(((unsigned long long)b >> 1) & 1) : 0; };')
    L += _ws_loader(ir, cfg, g, ws)
    L.append('  // consumer waves')
    L += [f'  f32x2 {_acc(gr, k)} = (f32x2)(0);' for si in range(len(plans)) for k in range(S)
          for gr in H.groups if gr[0] == si]
    L.append(f'  const int nplanes = ze - zb + {2 * RZ};')
    for nr in range(NR):
        for q in range(Q):
            L.append(f'  const unsigned rb_{nr}_{q} = (unsigned)((ybase + {nr}) * X + xbase + {4 * q}) * 2u;')
    if any(H.dpp_row(row) for row in rows):
        # element offset (from the lane's first cell) of its edge dword: lane 0 the wave's left neighbour,
        # lane 63 its right one, the others banks that stay distinct within each 32-lane group
        L.append(f'  const int eoff_ = 2 * (lane == 0 ? -1 : (lane == 63 ? {2 * Q * 64} : '
                 f'(lane < 32 ? lane - 1 : lane - 31))) - {CX} * lane;')
    L.append('  for (int j = 0; j < nplanes; ++j) {')
    L.append(f'    const int p = zb - {RZ} + j;')
    L.append(f'    {WS_CONSUMER_BARRIER}')
    if cfg.XO and len(stencil) == 1:
        # one stencil field: the rows that start on a half dword follow from ONE parity per plane and wave (its
        # first row's); the plane's reads are printed for both, so each row's realignment is static
        f0 = stencil[0]
        L.append(f'    const int par = ((ybase * X * {g["FG"][f0.name]["C"]}) + hpar({ws_plane_base(f0, RZ, "p")})) & 1;')
        names = sorted({_hname('A', fn, jr, d) for fn, jr in rows
                        for d in (range(-1, 2 * Q + 1) if H.dpp_row((fn, jr)) else H.dwords[(fn, jr)][1])})
        L.append('    f16x2 ' + ', '.join(names) + ';')
        for par in (1, 0):
            L.append(f'    {"if (par)" if par else "else"} {{')
            shmap = {(fn, jr): (par ^ ((jr & 1) if cfg.XO == 1 else 0)) for fn, jr in rows}
            L += _reads(H, '      ', 'A', f'j % {ws["NS"]}', False, shmap)
            L.append('    }')
    else:
        L += _reads(H, '    ', 'A', f'j % {ws["NS"]}', True)
    L += _compute(H, '    ', 'A')
    L.append('  }')
    L.append('}')
    return '\n'.join(L) + '\n'
