"""The ``zsum`` schedule: z-partial sums in register accumulators, each plane staged in LDS once."""
from dataclasses import dataclass

import numpy as np
import sympy as sp

from ...ps import Field
from ..printer import KernelExprPrinter
from .common import PRELUDE, _ctype, _split_offsets, _tag, flat_index, ncomp, retirement_lines, storage_ctype
from .config import MarchConfig
from .geometry import march_geometry, ws_geometry, zsum_plan
from .loader import WS_CONSUMER_BARRIER, _ws_loader
from .prelude import _march_prelude
from .zsum_half import _emit_zsum_half


@dataclass
class ZsumTables:
    """What ``emit_zsum`` prints from. ``taps``: the distinct taps of the arriving plane, (field, jr, cx, dx,
    component) → variable; ``lin_code[(si, dz, nr, c0)]``: plan ``si``'s terms constant × tap for the output ``dz``
    behind the plane, as (expression, symbol names), per row and column group (``lin_cols``: single columns, or with
    ``pk`` the column pairs of the packed fp32 form); ``rest_code[(si, nr, cx)]``: the centre-plane remainder per cell;
    ``point_fields``: the fields the remainders read at the cell; ``groups``: the accumulator groups (si, nr, c0);
    ``ct`` / ``at``: the C types of a value and of an accumulator."""
    ir: object
    cfg: object
    plans: list
    g: dict
    ct: str
    at: str
    pk: bool
    cells: list
    lin_cols: list
    groups: list
    taps: dict
    lin_code: dict
    rest_code: dict
    point_fields: list
    rest_any: bool

    def pr(self, expr, names):
        return KernelExprPrinter(self.ct, {**self.ir.symbol_names, **names}).doprint_expr(expr)

    def aname(self, group, k):
        """Accumulator variable of (plan, row, column group) and slot."""
        si, nr, c0 = group
        return f"a{si}_{k}_{_tag(nr)}_{c0 // 2 if self.pk else c0}"

    def cell_acc(self, si, k, nr, cx):
        """The accumulator (element) of one cell."""
        if not self.pk:
            return self.aname((si, nr, cx), k)
        return self.aname((si, nr, cx - cx % 2), k) + ('.x' if cx % 2 == 0 else '.y')

    def terms_of(self, group, dz):
        si, nr, c0 = group
        parts = self.lin_code.get((si, dz, nr, c0))
        return ' + '.join(f'({self.pr(e, n)})' for e, n in parts) if parts else None

    def tap_off(self, fname, jr, cx, dx, k):
        """Element offset of a tap from the lane's first cell in field fname's plane image."""
        fg = self.g['FG'][fname]
        return jr * fg['P'] + (64 * cx + dx) * fg['C'] + k


def _ksuf(k):
    return f"_k{k}" if k else ''


def _pair_name(fname, jr, j, dx, k):
    return f"tp_{fname}_{_tag(jr)}_{j}_{_tag(dx)}{_ksuf(k)}"


def _point_name(a, nr, cx):
    return f"pt_{a.field.name}_{_tag(nr)}_{cx}" + ('_i' + '_'.join(str(i) for i in a.index) if a.index else '')


def zsum_tables(ir, cfg, plans, g):
    """The ``ZsumTables`` of ``zsum_plan``'s ``plans`` on the tile of ``cfg``: planning only, no line is printed here."""
    ct =_ctype(ir.compute_dtype)
    stencil_set = set(ir.stencil_fields)
    CX, NR = cfg.CX, cfg.NR
    is3d = ir.ndim == 3
    cells = [(nr, cx) for nr in range(NR) for cx in range(CX)]
    taps = {}

    def tap(fname, jr, cx, dx, k=0):
        return taps.setdefault((fname, jr, cx, dx, k), f"t_{fname}_{_tag(jr)}_{cx}_{_tag(dx)}{_ksuf(k)}")

    pk = bool(cfg.PK) and ct == 'float' and CX % 2 == 0
    lin_code, rest_code = {}, {}
    lin_cols = [(cx,) for cx in range(CX)] if not pk else [(2 * j, 2 * j + 1) for j in range(CX // 2)]
    for si, pl in enumerate(plans):
        for nr in range(NR):
            for cols in lin_cols:
                for dz, terms in pl['lin'].items():
                    parts = []
                    for coeff, f, dy, dx, k in terms:
                        if pk:
                            v = _pair_name(f.name, nr + dy, cols[0] // 2, dx, k)
                            for cx in cols:
                                tap(f.name, nr + dy, cx, dx, k)
                        else:
                            v = tap(f.name, nr + dy, cols[0], dx, k)
                        sym = sp.Symbol(v)
                        parts.append((coeff * sym, {sym: v}))
                    lin_code[(si, dz, nr, cols[0])] = parts
        for nr, cx in cells:
            rest = pl['rest']
            names, repl = {}, {}
            for a in rest.free_symbols:
                if isinstance(a, Field.Access):
                    if a.field in stencil_set:
                        _, dy, dx = _split_offsets(a.offsets, is3d, cfg.VIEW2D)
                        v = tap(a.field.name, nr + dy, cx, dx, flat_index(a.field, a.index))
                    else:
                        v = _point_name(a, nr, cx)
                    sym = sp.Symbol(v)
                    repl[a] = sym
                    names[sym] = v
            rest_code[(si, nr, cx)] = (rest.xreplace(repl) if repl else rest, names)
    point_fields = sorted({a.field for pl in plans for a in pl['rest'].free_symbols
                           if isinstance(a, Field.Access) and a.field not in stencil_set}, key=lambda f: f.name)
    rest_any = any(rest_code[(si, nr, cx)][0] != 0 for si in range(len(plans)) for nr, cx in cells)
    groups = [(si, nr, cols[0]) for si in range(len(plans)) for nr in range(NR) for cols in lin_cols]
    return ZsumTables(ir, cfg, plans, g, ct, 'f32x2' if pk else ct, pk, cells, lin_cols, groups, taps, lin_code,
                      rest_code, point_fields, rest_any)


def tap_reads(T, ind):
    """The distinct taps of the staged plane, read once per thread through ``L_<field>``."""
    cfg, ct, FG = T.cfg, T.ct, T.g['FG']
    B = []
    named = sorted(T.taps.items(), key=lambda kv: kv[1])
    if not T.pk:
        return [f'{ind}const {ct} {var} = L_{fname}[{T.tap_off(fname, jr, cx, dx, k)}];'
                for (fname, jr, cx, dx, k), var in named]
    pairs = sorted({(fname, jr, cx // 2, dx, k) for (fname, jr, cx, dx, k) in T.taps})
    rx = max([-dx for _, _, _, dx, _ in pairs] + [0])
    # inline-asm paired reads need both offsets inside ds_read2_b32's 8-bit dword fields
    if cfg.AR and all((dx + rx) * FG[fname]['C'] + k + 64 * FG[fname]['C'] <= 255 for fname, _, _, dx, k in pairs):
        # one statement: every pair read of the plane, then the wait (registers never leave the asm
        # operand list between load and use, cdna_hip_programming.md 'What hipcc does not do' form i)
        bases = sorted({(fname, jr, j) for fname, jr, j, dx, k in pairs})
        for fname, jr, j in bases:
            B.append(f'{ind}const unsigned ab_{fname}_{_tag(jr)}_{j} = (unsigned)(size_t)'
                     f'(__attribute__((address_space(3))) const {ct}*)(L_{fname} + {T.tap_off(fname, jr, 2 * j, -rx, 0)});')
        ins = [f'"v"(ab_{fname}_{_tag(jr)}_{j})' for fname, jr, j in bases]
        outs, text = [], []
        for n, (fname, jr, j, dx, k) in enumerate(pairs):      # operands: the pairs, then the row bases
            v = _pair_name(fname, jr, j, dx, k)
            B.append(f'{ind}f32x2 {v};')
            C = FG[fname]['C']
            o0 = (dx + rx) * C + k
            text.append(f'ds_read2_b32 %{n}, %{len(pairs) + bases.index((fname, jr, j))} '
                        f'offset0:{o0} offset1:{o0 + 64 * C}')
            outs.append(f'"=&v"({v})')
        B.append(f'{ind}asm volatile("' + '\\n\\t'.join(text + ['s_waitcnt lgkmcnt(0)']) + '"')
        B.append(f'{ind}             : {", ".join(outs)}')
        B.append(f'{ind}             : {", ".join(ins)} : "memory");')
    else:
        for fname, jr, j, dx, k in pairs:
            o = T.tap_off(fname, jr, 2 * j, dx, k)
            v = _pair_name(fname, jr, j, dx, k)
            B.append(f'{ind}f32x2 {v}; {v}.x = L_{fname}[{o}]; {v}.y = L_{fname}[{o + 64 * FG[fname]["C"]}];')
    return B + [f'{ind}const {ct} {var} = {_pair_name(fname, jr, cx // 2, dx, k)}.' + ('x;' if cx % 2 == 0 else 'y;')
                for (fname, jr, cx, dx, k), var in named]


def rest_block(T, ind):
    """Centre-plane terms of output p. Only point-field reads need the domain guard: contributions
    to planes / cells outside [zb, ze) x [ylo, yhi) x [xlo, xhi) are never stored."""
    R = []
    if not T.rest_any:
        return R
    ct, plans, point_fields = T.ct, T.plans, T.point_fields
    rest_slot = T.g['RZ'] - 1 if T.g['RZ'] else 't'
    R.append(f'{ind}{{')
    if point_fields:
        R.append(f'{ind}  const i64 poff = (i64)p * YX;')
        R.append(f'{ind}  const bool zin = p >= zb && p < ze;')
    for nr, cx in T.cells:
        R.append(f'{ind}  {{')
        i2 = ind + '    '
        if point_fields:
            R.append(f'{ind}    const int y = ybase + {nr};')
            R.append(f'{ind}    const int x = xbase + {64 * cx};')
            R.append(f'{ind}    if (zin && y >= ylo && y < yhi && x >= xlo && x < xhi) {{')
            i2 = ind + '      '
            for f in point_fields:
                for a_ in sorted({a_ for pl in plans for a_ in pl['rest'].free_symbols
                                  if isinstance(a_, Field.Access) and a_.field == f}, key=str):
                    cell = '(poff + (i64)y * X + x)' + (f' * {ncomp(f)} + {flat_index(f, a_.index)}'
                                                          if f.index_dimensions else '')
                    R.append(f'{i2}const {ct} {_point_name(a_, nr, cx)} = ({ct})f_{f.name}[{cell}];')
        for si in range(len(plans)):
            expr, names = T.rest_code[(si, nr, cx)]
            if expr != 0:
                av = T.cell_acc(si, rest_slot, nr, cx)
                R.append(f'{i2}{av} = {av} + ' + ' + '.join(f'({T.pr(t_, names)})' for t_ in sp.Add.make_args(expr)) + ';')
        if point_fields:
            R.append(f'{ind}    }}')
        R.append(f'{ind}  }}')
    R.append(f'{ind}}}')
    return R


def store_block(T, ind, zexpr, val_of):
    """Guarded stores of output plane ``zexpr`` (if >= zb): ``val_of(si, nr, cx)`` = the value in the
    storage type."""
    cfg = T.cfg
    B = [f'{ind}if ({zexpr} >= zb) {{', f'{ind}  const i64 ooff = (i64)({zexpr}) * YX;']

    def dst_cell(pl):
        """Element index of output plan pl's cell — components interleaved."""
        C = ncomp(pl['field'])
        base = '(ooff + (i64)y * X + x)'
        return f'{base} * {C} + {pl["k"]}' if C > 1 else base
    for nr, cx in T.cells:
        B.append(f'{ind}  {{')
        B.append(f'{ind}    const int y = ybase + {nr};')
        B.append(f'{ind}    const int x = xbase + {64 * cx};')
        if cfg.XB:
            B.append(f'{ind}    const bool xin = x >= xlo && x < xhi;')
            B.append(f'{ind}    if (y >= ylo && y < yhi && x < X) {{')
        else:
            B.append(f'{ind}    if (y >= ylo && y < yhi && x >= xlo && x < xhi) {{')
        for si, pl in enumerate(T.plans):
            val = val_of(si, nr, cx)
            if cfg.XB:
                val = f"(xin ? {val} : ({storage_ctype(pl['field'])})0)"
            if cfg.NT_STORE:
                B.append(f'{ind}      __builtin_nontemporal_store({val}, f_{pl["field"].name} + {dst_cell(pl)});')
            else:
                B.append(f'{ind}      f_{pl["field"].name}[{dst_cell(pl)}] = {val};')
        B.append(f'{ind}    }}')
        B.append(f'{ind}  }}')
    B.append(f'{ind}}}')
    return B


def declare_accumulators(T, ind):
    return [f"{ind}{T.at} {T.aname((si, nr, cols[0]), k)} = ({T.at})(0);"
            for si in range(len(T.plans)) for k in range(2 * T.g['RZ']) for nr in range(T.cfg.NR) for cols in T.lin_cols]


def plane_body(T, ind, lds_of):
    """Statements of one plane ``p``: LDS taps, contributions to outputs p-RZ..p+RZ, store of
    output ``p - RZ``, accumulator retirement (``retirement_lines``). ``lds_of(f)`` = LDS pointer expression of
    field f's staged plane."""
    RZ = T.g['RZ']
    B = [f'{ind}const {T.ct}* L_{f.name} = {lds_of(f)} + lb_{f.name};' for f in T.ir.stencil_fields]
    B += tap_reads(T, ind)
    before, after = retirement_lines(ind, RZ, T.groups, T.aname, T.terms_of, f'({T.at})(0)', temp=f'{T.at} ')
    out_slot = 't' if RZ == 0 else 0
    B += before
    if RZ == 0:
        B += rest_block(T, ind)
    B += store_block(T, ind, f'p - {RZ}', lambda si, nr, cx: f"({storage_ctype(T.plans[si]['field'])})"
                     f"({T.cell_acc(si, out_slot, nr, cx)})")
    B += after
    if RZ > 0:
        B += rest_block(T, ind)
    return B


def emit_zsum(ir, name, cfg: MarchConfig):
    """z-partial-sum schedule for stencils linear in their off-centre planes (27-point boxes).

    The march ring re-reads every plane's (dy, dx) neighbourhood from LDS once per output plane
    it contributes to (three times for RZ=1). Here each plane ``p`` is staged in LDS ONCE, its
    distinct taps are read once per thread, and its contribution to each output plane
    ``p - dz`` is added into a per-cell register accumulator (``2·RZ`` of them, fused retirement);
    the output of plane ``p - RZ`` is complete and stored. LDS holds one plane per stencil field;
    the loop runs over ``zc + 2·RZ`` planes per chunk (same HBM traffic as the ring).
    """
    plans = zsum_plan(ir, cfg)
    if plans is None:
        raise ValueError('kernel is not eligible for the zsum schedule')
    g = march_geometry(ir, cfg)
    RZ, RY, H, TR, P = (g[k] for k in ('RZ', 'RY', 'H', 'TR', 'P'))
    stencil = ir.stencil_fields
    ws = ws_geometry(ir, cfg)
    if ir.periodic and (not ws or cfg.XM or cfg.XO or cfg.XB):
        # (the register-prefetch loads, the row-end fills and the x-border stores are the 'zeros' boundary)
        raise ValueError('periodic kernels take the zsum schedule only with the LDS-DMA loader on rows of whole '
                         '16-byte pieces (no XM / XO / XB config)')
    if ws and ws['kind'] == 'h':
        return _emit_zsum_half(ir, name, cfg, plans, g, ws)
    T = zsum_tables(ir, cfg, plans, g)
    lds_bytes = ws['lds_bytes'] if ws else \
        sum(TR * g['FG'][f.name]['P'] for f in stencil) * np.dtype(ir.compute_dtype).itemsize
    L = [PRELUDE]
    L.append(f"// zsum schedule: TX={cfg.TX} TY={cfg.TY} CX={cfg.CX} WX={cfg.WX} NR={cfg.NR} VE={cfg.VE}, "
             + (f"LDS-DMA loader wave, {ws['NS']}-slot plane ring, {ws['D']} planes in flight, " if ws
                else "one LDS plane per stencil field, ")
             + f"{max(1, 2 * RZ)} register accumulators per cell and output, "
             f"radius(z,y,x)=({RZ},{RY},{g['RX']}), "
             f"halo H={H}, pitch P={P}, LDS {lds_bytes} B" + (", packed fp32 column pairs" if T.pk else ""))
    L += _march_prelude(ir, name, cfg, g, {f.name: 1 for f in stencil}, ws=ws)
    if ws:
        L += _ws_loader(ir, cfg, g, ws)
        # consumer waves: one barrier per plane; plane j of the chunk sits in ring slot j % NS
        L += ['  // consumer waves'] + declare_accumulators(T, '  ')
        L += [f'  const int nplanes = ze - zb + {2 * RZ};',
              '  for (int j = 0; j < nplanes; ++j) {',
              f'    const int p = zb - {RZ} + j;',
              f'    const int slot = j % {ws["NS"]};',
              f'    {WS_CONSUMER_BARRIER}',
              '    {']
        L += plane_body(T, '      ', lambda f: f'lds_{f.name} + slot * {ws["F"][f.name]["SLOT"]}')
        return '\n'.join(L + ['    }', '  }', '}']) + '\n'

    L += declare_accumulators(T, '  ')
    # plane p + 1 is in flight in registers (set A) while plane p, stashed into the one LDS slot, is computed
    L += [f'  load_{f.name}(preA_{f.name}, zb - {RZ} + 0);' for f in stencil]
    L += [f'  for (int p0 = zb - {RZ}; p0 < ze + {RZ}; p0 += 1) {{', '    {', '    const int p = p0 + 0;']
    L += [f'    stash_{f.name}(preA_{f.name}, 0);' for f in stencil]
    L += ['    __syncthreads();', f'    if (p + 1 < ze + {RZ}) {{']
    L += [f'      load_{f.name}(preA_{f.name}, p + 1);' for f in stencil]
    L += ['    }', '    {']
    L += plane_body(T, '      ', lambda f: f'lds_{f.name}')
    L += ['    }', '    __syncthreads();',     # the single slot is overwritten by the next stash
          '    }', '  }', '}']
    return '\n'.join(L) + '\n'
