"""The ``march`` schedule: a ring of planes in LDS (register prefetch or LDS-DMA loader), one output plane per step."""
from ..printer import KernelExprPrinter
from .common import PRELUDE, _ctype, _split_offsets, _statements, _tag, flat_index, ncomp, storage_ctype
from .config import MarchConfig
from .geometry import march_geometry, pair_ok, ws_geometry
from .loader import WS_CONSUMER_BARRIER, _ws_loader
from .prelude import _march_prelude


def march_taps(ir, cfg, g):
    """``(cells, taps)``: the cells (nr, cx) a thread owns and its distinct taps, (field, dz, jr, cx, dx, k) → variable;
    jr = row relative to the thread's first row, k = the component of a vector field (interleaved in the plane image;
    0 for a scalar field); cx = the column (of cell pairs with PR). A lite field's taps behind the centre are the
    registers of its queue (``q_…``)."""
    stencil, lite = ir.stencil_fields, g['lite']
    stencil_set = set(stencil)
    is3d = ir.ndim == 3
    cells = [(nr, cx) for nr in range(cfg.NR) for cx in range(cfg.CX // 2 if cfg.PR else cfg.CX)]
    taps = {}
    for nr, cx in cells:
        for r in ir.reads:
            if r.field not in stencil_set:
                continue
            dz, dy, dx = _split_offsets(r.offsets, is3d, cfg.VIEW2D)
            taps.setdefault((r.field.name, dz, nr + dy, cx, dx, flat_index(r.field, r.index)), None)
    for f in (lite if g['RZ'] > 0 else ()):   # lite fields: the centre taps feed the register queue
        for k in range(ncomp(f)):
            for nr, cx in cells:
                taps.setdefault((f.name, 0, nr, cx, 0, k), None)
    for key in taps:
        fname, dz, jr, cx, dx, k = key
        ck = f'_c{k}' if ncomp(next(f for f in stencil if f.name == fname)) > 1 else ''
        if dz < 0 and any(f.name == fname for f in lite):
            taps[key] = f"q_{fname}_{-dz}_{_tag(jr)}_{cx}{ck}"
        else:
            taps[key] = f"t_{fname}_{_tag(dz)}_{_tag(jr)}_{cx}_{_tag(dx)}{ck}"
    return cells, taps


def _lds_val(cfg, arr, idx, off, C=1):
    """A lane's value at ``arr[idx + off]`` (``off`` an int): the pair (off, off + C) with PR (C: the field's
    components, interleaved — the pair's second cell is C elements on)."""
    if cfg.PR:
        return f'(f32x2){{{arr}[{idx} + {off}], {arr}[{idx} + {off + C}]}}'
    return f'{arr}[{idx} + {off}]'


def _cks(f):
    """Component suffixes of a (lite) field's register queue: '' for a scalar field."""
    return [f'_c{c}' for c in range(ncomp(f))] if ncomp(f) > 1 else ['']


def _rotate_lines(g, cells, indent, center_of):
    """The lite fields' register queues move on by one plane. ``center_of(f, nr, cx, c)``: the value of component
    ``c`` of the lane's cell (nr, cx) in plane z."""
    RZ = g['RZ']
    out = []
    if RZ == 0:
        return out
    for f in sorted(g['lite'], key=lambda f: f.name):
        for k in range(RZ, 1, -1):
            for nr, cx in cells:
                for ck in _cks(f):
                    out.append(f"{indent}q_{f.name}_{k}_{_tag(nr)}_{cx}{ck} = q_{f.name}_{k - 1}_{_tag(nr)}_{cx}{ck};")
        for nr, cx in cells:
            for c, ck in enumerate(_cks(f)):
                out.append(f"{indent}q_{f.name}_1_{_tag(nr)}_{cx}{ck} = {center_of(f, nr, cx, c)};")
    return out


def emit_march(ir, name, cfg: MarchConfig):
    """The z-marching stencil kernel (see the package docstring).

    Per step ``z`` (one plane of axis 0) a workgroup: stores the prefetched plane
    ``z+RZ`` into its LDS ring slot, barrier, issues the global loads of plane
    ``z+RZ+PD``, reads every distinct tap of its cells from LDS (or, for planes behind
    the centre of a "lite" field, from registers), evaluates the statements, stores
    the outputs, barrier.
    """
    if ir.ndim not in (2, 3):
        raise ValueError('march schedule needs 2-D or 3-D fields')
    g = march_geometry(ir, cfg)
    RZ, RY, H, P = (g[k] for k in ('RZ', 'RY', 'H', 'P'))
    slots, lite = g['slots'], g['lite']
    printer = KernelExprPrinter(_ctype(ir.compute_dtype), ir.symbol_names)
    stencil = ir.stencil_fields
    PR = bool(cfg.PR)
    if PR and (cfg.CX % 2 or not pair_ok(ir, vectors=bool(cfg.WS))):
        raise ValueError('PR=1: packed cell pairs need an even CX and fp32 statements of +, ×, integer powers '
                         '(hip_emitter.pair_ok; vector fields on the LDS-DMA ring only)')
    vt = 'f32x2' if PR else _ctype(ir.compute_dtype)
    cells, taps = march_taps(ir, cfg, g)
    ws = ws_geometry(ir, cfg) if cfg.WS else None
    if ir.periodic and not ws:
        raise ValueError('periodic kernels take the march ring only with the LDS-DMA loader (wrapped plane loads)')
    if not ws and any(ncomp(f) > 1 for f in stencil):
        raise ValueError('vector stencil fields take the LDS-DMA plane ring (WS) or the zsum schedule')
    L = [PRELUDE]
    if ws:
        slots = {f.name: ws['F'][f.name]['NS'] for f in stencil}
    L.append(f"// march schedule: TX={cfg.TX} TY={cfg.TY} CX={cfg.CX} WX={cfg.WX} NR={cfg.NR} VE={cfg.VE} PD={cfg.PD} "
             f"ring slots={slots} (lite={sorted(f.name for f in lite)}), radius(z,y,x)=({RZ},{RY},{g['RX']}), "
             f"halo H={H}, pitch P={P}, LDS {ws['lds_bytes'] if ws else g['lds_bytes']} B"
             + (f", LDS-DMA loader wave, {ws['D']} planes in flight" if ws else ''))
    L += _march_prelude(ir, name, cfg, g, slots, ws=ws, lane_stride=2 if PR else 1)
    for f in sorted(lite, key=lambda f: f.name):
        for k in range(1, RZ + 1):
            for nr, cx in cells:
                for ck in _cks(f):
                    L.append(f"  {vt} q_{f.name}_{k}_{_tag(nr)}_{cx}{ck} = ({vt})0;")
    L += _march_ws_body(ir, cfg, g, ws, cells, taps, printer) if ws else _march_reg_body(ir, cfg, g, cells, taps, printer)
    L.append('}')
    return '\n'.join(L) + '\n'


def _march_reg_body(ir, cfg, g, cells, taps, printer):
    """``emit_march`` on the register-prefetch ring: ``PD`` planes in flight in register sets A / B."""
    RZ, TR, P = g['RZ'], g['TR'], g['P']
    lite, stencil, PD = g['lite'], ir.stencil_fields, cfg.PD
    ct = _ctype(ir.compute_dtype)
    CW = 128 if cfg.PR else 64
    # prologue: planes zb-RZ .. zb+RZ-1 into the rings (lite fields: planes behind zb into registers)
    L = [f'  for (int p = zb - {RZ}; p < zb + {RZ}; ++p) {{']
    L += [f'    load_{f.name}(preA_{f.name}, p);' for f in stencil]
    L += [f'    stash_{f.name}(preA_{f.name}, slot_{f.name}(p));' for f in stencil]
    if lite:
        L.append('    if (p < zb) {')
        L.append('      __syncthreads();')
        L += _rotate_lines(g, cells, '      ', lambda f, nr, cx, c:
                           _lds_val(cfg, f"lds_{f.name}", f"slot_{f.name}(p) * {TR * P} + lbase", nr * P + cx * CW))
        L.append('      __syncthreads();')
        L.append('    }')
    L.append('  }')
    for i, s_ in enumerate(['A', 'B'][:PD]):
        L.append(f'  if (zb + {i} < ze) {{')
        L += [f'    load_{f.name}(pre{s_}_{f.name}, zb + {RZ + i});' for f in stencil]
        L.append('  }')

    def step(zexpr, s_):
        ind = '    '
        out = [f'{ind}stash_{f.name}(pre{s_}_{f.name}, slot_{f.name}({zexpr} + {RZ}));' for f in stencil]
        out.append(f'{ind}__syncthreads();')
        out.append(f'{ind}if ({zexpr} + {PD} < ze) {{')
        out += [f'{ind}  load_{f.name}(pre{s_}_{f.name}, {zexpr} + {PD + RZ});' for f in stencil]
        out.append(f'{ind}}}')
        out.append(f'{ind}{{')
        ind2 = ind + '  '
        out.append(f'{ind2}const int zz = {zexpr};')
        out.append(f'{ind2}const i64 zoff = (i64)zz * YX;')
        for f in stencil:
            lo = 0 if f in lite else -RZ
            for dz in range(lo, RZ + 1):
                out.append(f'{ind2}const {ct}* L_{f.name}_{_tag(dz)} = lds_{f.name} + slot_{f.name}(zz + ({dz})) * '
                           f'{TR * P} + lbase;')
        out += _march_cells(ir, cfg, g, taps, printer, ind2, split=bool(cfg.PR) and bool(cfg.SFAST))
        out += _rotate_lines(g, cells, ind2, lambda f, nr, cx, c: taps[(f.name, 0, nr, cx, 0, c)])
        out.append(f'{ind}}}')
        out.append(f'{ind}__syncthreads();')
        return out

    if PD == 1:
        L.append('  for (int z = zb; z < ze; ++z) {')
        L += step('z', 'A')
        L.append('  }')
    else:
        L.append('  for (int z = zb; z < ze; z += 2) {')
        L += step('z', 'A')
        L.append('    if (z + 1 < ze) {')
        L += ['  ' + x for x in step('(z + 1)', 'B')]
        L.append('    }')
        L.append('  }')
    return L


def _march_ws_body(ir, cfg, g, ws, cells, taps, printer):
    """``emit_march`` on the LDS-DMA ring (``ws_geometry`` kind ``'ring'``): the loader wave (``_ws_loader``) puts
    plane ``j`` of the chunk (``zb − RZ + j``) into slot ``j % NS_f`` of field ``f``'s ring, ``D`` planes ahead;
    the compute waves pass one barrier per plane — planes behind ``zb`` feed the lite fields' register queues,
    from plane ``zb + RZ`` on each barrier completes output plane ``z = zb + j − 2·RZ``."""
    RZ, lite = g['RZ'], g['lite']
    CW = 128 if cfg.PR else 64
    L = _ws_loader(ir, cfg, g, ws)
    L.append('  // compute waves')
    L.append(f'  const int nplanes = ze - zb + {2 * RZ};')
    L.append('  for (int j = 0; j < nplanes; ++j) {')
    L.append(f'    {WS_CONSUMER_BARRIER}')
    FG = g['FG']

    def lane_base(f):
        """The lane's first cell in field f's image (``lbase`` for a scalar field: the same expression)."""
        return 'lbase' if FG[f.name]['C'] == 1 else f'lb_{f.name}'
    if RZ and lite:
        L.append(f'    if (j < {RZ}) {{')
        L += _rotate_lines(g, cells, '      ', lambda f, nr, cx, c:
                           _lds_val(cfg, f"lds_{f.name}", f"(j % {ws['F'][f.name]['NS']}) * {ws['F'][f.name]['SLOT']} + "
                                    f"{lane_base(f)}", nr * FG[f.name]['P'] + cx * CW * FG[f.name]['C'] + c,
                                    FG[f.name]['C']))
        L.append('      continue;')
        L.append('    }')
    if RZ:
        L.append(f'    if (j < {2 * RZ}) continue;')
    ind2 = '    '
    L.append(f'{ind2}const int zz = zb + j - {2 * RZ};')
    L.append(f'{ind2}const i64 zoff = (i64)zz * YX;')
    for f in ir.stencil_fields:
        lo = 0 if f in lite else -RZ
        NS, SLOT = ws['F'][f.name]['NS'], ws['F'][f.name]['SLOT']
        for dz in range(lo, RZ + 1):
            L.append(f'{ind2}const {ws["lds_type"]}* L_{f.name}_{_tag(dz)} = lds_{f.name} + ((j - {RZ - dz}) % {NS}) * '
                     f'{SLOT} + {lane_base(f)};')
    L += _march_cells(ir, cfg, g, taps, printer, ind2, split=bool(cfg.SFAST),
                      lds_half=ws['lds_type'] == '_Float16')
    L += _rotate_lines(g, cells, ind2, lambda f, nr, cx, c: taps[(f.name, 0, nr, cx, 0, c)])
    L.append('  }')
    return L


def _cell_at(field, idx):
    """Element of ``field`` for component ``idx`` of the cell ``cell`` (components fastest; ``cell`` for a scalar)."""
    C = ncomp(field)
    return 'cell' if C == 1 else f'cell * {C} + {flat_index(field, idx)}'


def _march_cells(ir, cfg, g, taps, printer, ind2, split=False, lds_half=False):
    """The compute part of one march step: every distinct LDS tap of the thread's cells (through the plane pointers
    ``L_<field>_<dz>``), then per cell the statements and guarded stores of output plane ``zz``. The scalar and the
    packed-pair form (``_scalar_cells`` / ``_pair_cells``) supply the tap declarations, the guards, how a point read is
    bound and the store; the per-cell frame and the fast / guarded split are printed here."""
    pair = bool(cfg.PR)
    out, guards, guard, point_read, store = (_pair_cells if pair else _scalar_cells)(ir, cfg, g, taps, ind2, lds_half)
    vt = 'f32x2' if pair else _ctype(ir.compute_dtype)
    ncol, cw = (cfg.CX // 2, 128) if pair else (cfg.CX, 64)
    stencil_set = set(ir.stencil_fields)
    is3d = ir.ndim == 3

    def cells(ind, checked):
        B = []
        for cx in range(ncol):
            for nr in range(cfg.NR):
                B.append(f'{ind}{{')
                B.append(f'{ind}  const int y = ybase + {nr};')
                B.append(f'{ind}  const int x = xbase + {cx * cw};')
                if checked:
                    B += [f'{ind}  {line}' for line in guards]
                B.append(f'{ind}  if ({guard if checked else "true"}) {{')
                B.append(f'{ind}    const i64 cell = zoff + (i64)y * X + x;')
                for r in ir.reads:
                    if r.field in stencil_set:
                        dz, dy, dx = _split_offsets(r.offsets, is3d, cfg.VIEW2D)
                        B.append(f'{ind}    const {vt} {r.var} = '
                                 f'{taps[(r.field.name, dz, nr + dy, cx, dx, flat_index(r.field, r.index))]};')
                    else:
                        B.append(f'{ind}    const {vt} {r.var} = {point_read(r, checked)};')
                B += _statements(ir, printer, ind + '    ', lambda field, offs, idx, code:
                                 store(field, idx, code, ind + '    ', checked), vt=vt if pair else None)
                B.append(f'{ind}  }}')
                B.append(f'{ind}}}')
        return B
    if not split:
        return out + cells(ind2, True)
    # a wave whose cells all lie inside the written box (wave-uniform test): no per-cell guards, so the compiler
    # schedules the cells' arithmetic and stores as one block instead of one exec-masked branch per cell
    out.append(f'{ind2}if (ybase >= ylo && ybase + {cfg.NR} <= yhi && x0 + wx * {64 * cfg.CX} >= xlo && '
               f'x0 + wx * {64 * cfg.CX} + {64 * cfg.CX} <= xhi) {{')
    out += cells(ind2 + '  ', False)
    out.append(f'{ind2}}} else {{')
    out += cells(ind2 + '  ', True)
    out.append(f'{ind2}}}')
    return out


def _scalar_cells(ir, cfg, g, taps, ind2, lds_half):
    """One cell per lane and column: ``(tap declarations, guard declarations, guard, point_read, store)``."""
    ct = _ctype(ir.compute_dtype)
    FG = g['FG']
    out = []
    # every distinct LDS tap of the thread's cells first (reading each right before its first use
    # saves VGPRs but measured slower: 1.69 vs 1.60 ms at 1024³, profiles/r01_tune_7pt_lazy_ab.log)
    for key, var in sorted(taps.items(), key=lambda kv: kv[1]):
        if var.startswith('q_'):
            continue
        fname, dz, jr, cxx, dx, k = key
        C = FG[fname]['C']         # components interleaved in the image: element (x, k) at x·C + k, rows P_f apart
        out.append(f'{ind2}const {ct} {var} = L_{fname}_{_tag(dz)}[{jr * FG[fname]["P"] + (cxx * 64 + dx) * C + k}];')

    def point_read(r, checked):
        return f'({ct})f_{r.field.name}[{_cell_at(r.field, r.index)}]'

    def store(field, idx, code, i, checked):
        t = storage_ctype(field)
        at = _cell_at(field, idx)
        if cfg.NT_STORE:
            return f'{i}__builtin_nontemporal_store(({t})({code}), f_{field.name} + {at});'
        return f'{i}f_{field.name}[{at}] = ({t})({code});'
    return out, [], 'y >= ylo && y < yhi && x >= xlo && x < xhi', point_read, store


def _pair_cells(ir, cfg, g, taps, ind2, lds_half):
    """``_scalar_cells`` with ``PR``: a lane owns the cell pairs (x, x + 1) of its columns (128 apart), every tap is an
    ``f32x2`` read as one ``ds_read2_b32``, the statements run on ``f32x2`` (packed fp32: two cells per VALU
    instruction), and each output pair is one 8-byte (fp32) / 4-byte (fp16) store where the pair is aligned — a
    wave-uniform test (a row's pairs all share the parity of its first cell) — else two element stores. Boundary
    waves guard each cell of a pair on its own."""
    FG = g['FG']
    out = []
    dwords = {}
    for key, var in sorted(taps.items(), key=lambda kv: kv[1]):
        if var.startswith('q_'):
            continue
        fname, dz, jr, cp, dx, k = key
        C = FG[fname]['C']          # vector fields: components interleaved, the pair's second cell C elements on
        o = jr * FG[fname]['P'] + (cp * 128 + dx) * C + k
        Lp = f'L_{fname}_{_tag(dz)}'
        if not lds_half:
            out.append(f'{ind2}const f32x2 {var} = (f32x2){{{Lp}[{o}], {Lp}[{o + C}]}};')
            continue
        if C > 1:
            # (fp16 vector image: the two halves are C apart; the compiler merges a lane's adjacent reads — its cells'
            # elements are contiguous from an even offset)
            out.append(f'{ind2}const f32x2 {var} = (f32x2){{(float){Lp}[{o}], (float){Lp}[{o + C}]}};')
            continue
        # fp16 image: the lane's element offsets are even (image pitch, halo and lane base even), so a pair at an
        # even offset is one dword; an odd pair takes the high half of the dword before it and the low half of
        # the dword after it (one v_perm). Each dword is read once per step.
        def dw(e, Lp=Lp):
            k = (Lp, e)
            if k not in dwords:
                dwords[k] = f'd_{Lp[2:]}_{_tag(e)}'
                out.append(f'{ind2}const f16x2 {dwords[k]} = *(const f16x2*)({Lp} + {e});')
            return dwords[k]
        h = dw(o) if o % 2 == 0 else f'__builtin_shufflevector({dw(o - 1)}, {dw(o + 1)}, 1, 2)'
        out.append(f'{ind2}const f32x2 {var} = __builtin_convertvector({h}, f32x2);')

    def point_read(r, checked):
        C, e0 = ncomp(r.field), _cell_at(r.field, r.index)
        e1 = f'(cell + 1) * {C} + {flat_index(r.field, r.index)}' if C > 1 else 'cell + 1'
        if checked:
            return (f'(f32x2){{in0 ? (float)f_{r.field.name}[{e0}] : 0.0f, '
                    f'in1 ? (float)f_{r.field.name}[{e1}] : 0.0f}}')
        return f'(f32x2){{(float)f_{r.field.name}[{e0}], (float)f_{r.field.name}[{e1}]}}'

    def store(field, idx, code, _i, checked):
        t = storage_ctype(field)
        p = f'f_{field.name}'
        S = [f'{_i}{{', f'{_i}  const f32x2 v_ = (f32x2)({code});']
        if t == 'float':
            pv, pt = 'v_', 'f32x2'
        else:
            S.append(f'{_i}  const f16x2 h_ = __builtin_convertvector(v_, f16x2);')
            pv, pt = 'h_', 'f16x2'
        C = ncomp(field)
        if C > 1:
            # vector field: the pair's two elements are C apart — two element stores
            k = flat_index(field, idx)
            e0, e1 = f'cell * {C} + {k}', f'(cell + 1) * {C} + {k}'
            if checked:
                S += [f'{_i}  if (in0) {p}[{e0}] = {pv}.x;', f'{_i}  if (in1) {p}[{e1}] = {pv}.y;']
            elif cfg.NT_STORE:
                S += [f'{_i}  __builtin_nontemporal_store({pv}.x, {p} + {e0});',
                      f'{_i}  __builtin_nontemporal_store({pv}.y, {p} + {e1});']
            else:
                S += [f'{_i}  {p}[{e0}] = {pv}.x;', f'{_i}  {p}[{e1}] = {pv}.y;']
        elif checked:
            S += [f'{_i}  if (in0) {p}[cell] = {pv}.x;', f'{_i}  if (in1) {p}[cell + 1] = {pv}.y;']
        else:
            al = 8 if t == 'float' else 4
            st = (f'__builtin_nontemporal_store({pv}, ({pt}*)({p} + cell));' if cfg.NT_STORE
                  else f'*({pt}*)({p} + cell) = {pv};')
            S += [f'{_i}  if ((__builtin_amdgcn_readfirstlane((unsigned)(size_t)({p} + cell)) & {al - 1}) '
                  f'== 0) {st}',
                  f'{_i}  else {{ {p}[cell] = {pv}.x; {p}[cell + 1] = {pv}.y; }}']
        S.append(f'{_i}}}')
        return '\n'.join(S)
    guards = ['const bool yin = y >= ylo && y < yhi;',
              'const bool in0 = yin && x >= xlo && x < xhi, in1 = yin && x + 1 >= xlo && x + 1 < xhi;']
    return out, guards, 'in0 || in1', point_read, store
