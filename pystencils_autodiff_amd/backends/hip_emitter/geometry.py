"""Which kernels a marching schedule takes and the static sizes it is compiled with: tile and ring geometry,
the packed-pair and half-ring eligibility tests, and the zsum decomposition of the stores (``zsum_plan``)."""
import numpy as np
import sympy as sp

from ...ps import Field
from .common import _ctype, _split_offsets, flat_index, ncomp, storage_ctype


def lite_fields(ir, cfg):
    """Stencil fields whose planes behind the centre (dz < 0) are only read at (dy, dx) = (0, 0):
    those planes live in registers, the LDS ring keeps ``RZ+1`` planes instead of ``2·RZ+1``."""
    is3d = ir.ndim == 3
    out = set()
    for f in ir.stencil_fields:
        ok = True
        for r in ir.reads:
            if r.field == f:
                dz, dy, dx = _split_offsets(r.offsets, is3d, cfg.VIEW2D)
                if dz < 0 and (dy, dx) != (0, 0):
                    ok = False
        if ok:
            out.add(f)
    return out


def pair_ok(ir, vectors=False):
    """Kernels the packed-pair form (``MarchConfig.PR``) can evaluate on ``f32x2``: fp32 arithmetic, scalar fields
    (``vectors``: also fields of one index dimension, components interleaved — the LDS-DMA ring's pairs), and
    statements made of +, ×, integer powers, taps, parameters and numbers only (functions, selects and comparisons
    have no vector form here)."""
    if np.dtype(ir.compute_dtype) != np.float32:
        return False
    if any(ncomp(f) > 1 and (not vectors or f.index_dimensions != 1) for f in ir.fields):
        return False
    for rhs in [r for _, r in ir.subexpressions] + [s[3] for s in ir.stores]:
        for node in sp.preorder_traversal(sp.sympify(rhs)):
            if isinstance(node, (sp.Symbol, sp.Number, sp.NumberSymbol, sp.Add, sp.Mul)):
                continue
            if isinstance(node, sp.Pow) and node.exp.is_Integer:
                continue
            return False
    return True


def march_geometry(ir, cfg):
    """Static sizes the kernel is compiled with (radii in (z, y, x) of the 3-D view). ``FG`` holds each
    stencil field's plane image: ``C`` components per cell, row pitch ``P = (TX + 2H)·C`` elements,
    ``NCH`` vectors per row, ``NCHUNK`` vectors per plane, ``CPT`` vectors per thread."""
    if ir.ndim == 3:
        rz, ry, rx = ir.radius
    elif cfg.VIEW2D == 'yx':
        rz, (ry, rx) = 0, ir.radius
    else:
        rz, rx = ir.radius
        ry = 0
    ve = cfg.VE
    H = max(ve, -(-rx // ve) * ve) if rx > 0 else ve
    TR = cfg.TY + 2 * ry
    P = cfg.TX + 2 * H
    NCH = P // ve
    NCHUNK = TR * NCH
    CPT = -(-NCHUNK // cfg.NT)
    lite = lite_fields(ir, cfg)
    if cfg.ZSUM:
        slots = {f.name: 1 for f in ir.stencil_fields}
    else:
        slots = {f.name: (rz + 1 if f in lite else 2 * rz + 1) for f in ir.stencil_fields}
    FG = {}
    for f in ir.stencil_fields:
        C = ncomp(f)
        Pf = P * C
        FG[f.name] = dict(C=C, P=Pf, NCH=Pf // ve, NCHUNK=TR * (Pf // ve), CPT=-(-(TR * (Pf // ve)) // cfg.NT))
    lds_bytes = sum(slots[f.name] * TR * FG[f.name]['P'] for f in ir.stencil_fields) * \
        np.dtype(ir.compute_dtype).itemsize
    return dict(RZ=rz, RY=ry, RX=rx, H=H, S=2 * rz + 1, TR=TR, P=P, NCH=NCH, NCHUNK=NCHUNK, CPT=CPT,
                slots=slots, lite=lite, lds_bytes=lds_bytes, FG=FG)


def ws_geometry(ir, cfg):
    """LDS-DMA ring of the warp-specialised zsum schedule, or ``None`` if it does not apply.

    The loader wave copies a plane's tile image (``TR × P`` elements, rows contiguous, so one
    wave-instruction's 64 × 16 bytes land lane-linear) into ring slot ``j % NS`` with ``NI``
    ``buffer_load_dwordx4 … lds`` per stencil field. Pieces outside the plane (x / y halo at the
    domain edge, absent halo planes) use out-of-range offsets or a zero-record descriptor: the
    hardware writes zeros, which is the 'zeros' boundary. A periodic kernel's pieces wrap instead (the same image
    from wrapped source offsets, ``_ws_piece_offsets``; absent halo planes are the kernel's own far planes). Needs
    16-byte vectors of a storage type equal to the compute type.

    Without ``ZSUM`` (stencils that are not linear off the centre plane: products of taps, transcendental
    functions of neighbours) the same loader feeds the plane ring of ``emit_march`` (kind ``'ring'``): field
    ``f`` keeps ``NS_f = D + 2·RZ + 1`` slots (``D + RZ + 1`` for a "lite" field, whose planes behind the centre
    live in registers) — the planes the compute waves read at step ``z`` plus the ``D`` in flight."""
    if cfg.WS and not cfg.ZSUM:
        return _ring_ws_geometry(ir, cfg)
    if not (cfg.WS and cfg.ZSUM) or ir.ndim not in (2, 3) or cfg.NW != 4:
        return None
    stencil = ir.stencil_fields
    esize = np.dtype(ir.compute_dtype).itemsize
    ssizes = {np.dtype(f.dtype.numpy_dtype).itemsize for f in stencil}
    if len(ssizes) != 1 or cfg.VE * next(iter(ssizes)) != 16:
        return None
    g = march_geometry(ir, cfg)
    FG = g['FG']
    NIs = {f.name: -(-FG[f.name]['NCHUNK'] // 64) for f in stencil}
    per_plane = sum(NIs.values())
    if all(storage_ctype(f) == _ctype(ir.compute_dtype) for f in stencil):
        # LDS-DMA straight into a ring of D+1 slots of the storage type
        D = max(1, min(cfg.D, 1 + 63 // per_plane)) if per_plane <= 63 else 1
        NS = D + 1
        F = {n: dict(NI=ni, SLOT=ni * 1024 // esize) for n, ni in NIs.items()}
        return dict(kind='dma', D=D, NS=NS, F=F, per_plane=per_plane, esize=esize, block=320,
                    lds_type=_ctype(ir.compute_dtype), lds_bytes=sum(NS * v['SLOT'] * esize for v in F.values()))
    if half_ring_ok(ir, cfg):
        # fp16 storage, fp32 arithmetic: the raw planes in a ring of D+1 fp16 slots; the compute waves read
        # their taps as fp16 pairs and convert in registers (no convert pass, no second LDS plane)
        ssize = next(iter(ssizes))
        D = max(1, min(cfg.D, 1 + 63 // per_plane)) if per_plane <= 63 else 1
        NS = D + 1
        F = {n: dict(NI=ni, SLOT=ni * 1024 // ssize) for n, ni in NIs.items()}
        return dict(kind='h', D=D, NS=NS, F=F, per_plane=per_plane, esize=ssize, block=320,
                    lds_type=storage_ctype(stencil[0]), lds_bytes=sum(NS * v['SLOT'] * ssize for v in F.values()))
    return None


def _ring_ws_geometry(ir, cfg):
    """``ws_geometry`` of the LDS-DMA plane ring of ``emit_march`` (3-D, scalar or one-index-dimension vector stencil
    fields whose storage type is the compute type, 16-byte pieces, rows of whole pieces), or ``None``. (fp16 planes in
    the ring, each tap read as a half and converted, measured 1.7x slower than the register-prefetch ring that stores
    fp32 images: varcoef 768³ fwd 1.48 vs 0.89 ms, bwd 3.3-4.4 vs 2.29 ms, profiles/r05_ring16_tiles.log — one
    ds_read_u16 per tap, no read2 pairing. Scalar fp16 fields therefore take it only as cell pairs (PR); vector
    fields, which the register ring does not take, take it per tap: 2x over one thread per cell.)"""
    if not (ir.ndim == 3 or (ir.ndim == 2 and cfg.VIEW2D == 'zy')) or cfg.NW not in (4, 8) or cfg.XM or cfg.XO:
        return None            # (2-D fields: marching along axis 0, rows as the ring's planes)
    stencil = ir.stencil_fields
    if not stencil:
        return None
    stypes = {storage_ctype(f) for f in stencil}
    esize = np.dtype(stencil[0].dtype.numpy_dtype).itemsize
    # fp16 planes with fp32 arithmetic: only with packed cell pairs (PR), whose taps are whole dwords of the image
    # (one ds_read_b32 and two conversions per pair of cells, odd pairs by one v_perm of two dwords)
    # (vector fields in fp16: the same ring of fp16 images, each tap read as one half and converted — the register ring
    # takes no vector fields, so the alternative is one thread per cell)
    half = stypes == {'_Float16'} and _ctype(ir.compute_dtype) == 'float' and (bool(cfg.PR) or ir.has_index_dims)
    if (stypes != {_ctype(ir.compute_dtype)} and not half) or cfg.VE * esize != 16:
        return None
    if ir.has_index_dims and any(len(f.index_shape) > 1 for f in ir.fields if f.index_dimensions):
        return None                         # vector fields (one index dimension, components interleaved) only
    g = march_geometry(ir, cfg)
    NIs = {f.name: -(-g['FG'][f.name]['NCHUNK'] // 64) for f in stencil}
    per_plane = sum(NIs.values())
    if per_plane > 63:
        return None
    D = max(1, min(cfg.D, 1 + 63 // per_plane))
    F = {f.name: dict(NI=NIs[f.name], SLOT=NIs[f.name] * 1024 // esize,
                      NS=D + (g['RZ'] + 1 if f in g['lite'] else 2 * g['RZ'] + 1)) for f in stencil}
    return dict(kind='ring', D=D, NS=max(v['NS'] for v in F.values()), F=F, per_plane=per_plane, esize=esize,
                block=64 * (cfg.NW + 1), lds_type=next(iter(stypes)),
                lds_bytes=sum(v['NS'] * v['SLOT'] * esize for v in F.values()))


def half_ring_ok(ir, cfg):
    """The half-precision ring (``ws_geometry`` kind ``'h'``) applies: every field fp16 storage with fp32
    arithmetic, scalar fields, stores at offset 0 that are pure sums of constant × tap (no centre-plane
    remainder, no point fields), CX a multiple of 4 (a lane owns CX x-adjacent cells, FMAs pair cells
    (x, x+2) and (x+1, x+3)), 16-byte DMA pieces."""
    if cfg.CX % 4 or cfg.VE != 8 or _ctype(ir.compute_dtype) != 'float' or ir.ndim != 3:
        return False
    if any(storage_ctype(f) != '_Float16' or ncomp(f) != 1 for f in ir.fields):
        return False
    stencil = set(ir.stencil_fields)
    if any(f not in stencil for f in ir.fields_read):
        return False
    plans = zsum_plan(ir, cfg)
    return plans is not None and all(pl['rest'] == 0 for pl in plans)


def zsum_plan(ir, cfg):
    """Decompose every store as ``Σ_dz Σ_taps c·tap(plane z+dz) + rest(plane z)``.

    Eligible when every term that reads a stencil field off the centre plane (dz != 0) is a
    constant (number / scalar parameter) times ONE such tap — true for every linear stencil and
    its TF-MAD adjoint. ``rest`` may be any expression of centre-plane taps and point fields.
    Returns ``None`` if the kernel is not eligible.
    """
    if ir.ndim not in (2, 3):
        return None
    is3d = ir.ndim == 3
    stencil = set(ir.stencil_fields)
    subs = {}
    for sym, rhs in ir.subexpressions:
        subs[sym] = rhs.xreplace(subs) if subs else rhs
    plans = []
    for field, offs, idx, rhs in ir.stores:
        if any(o != 0 for o in offs):
            return None
        full = sp.expand(rhs.xreplace(subs) if subs else rhs)
        lin, rest = {}, []
        for term in sp.Add.make_args(full):
            taps_ = [a for a in term.free_symbols if isinstance(a, Field.Access) and a.field in stencil]
            off_plane = [a for a in taps_ if _split_offsets(a.offsets, is3d, cfg.VIEW2D)[0] != 0]
            coeff = sp.simplify(term / taps_[0]) if len(taps_) == 1 else None
            linear = coeff is not None and not coeff.has(taps_[0]) and \
                not any(isinstance(a, Field.Access) for a in coeff.free_symbols)
            if not linear:
                if off_plane:
                    return None              # nonlinear in an off-centre plane: not eligible
                rest.append(term)            # centre-plane remainder, evaluated per cell
                continue
            # constant x one tap (any plane, centre included): a fused multiply-add into the accumulator
            dz, dy, dx = _split_offsets(taps_[0].offsets, is3d, cfg.VIEW2D)
            lin.setdefault(dz, []).append((coeff, taps_[0].field, dy, dx, flat_index(taps_[0].field, taps_[0].index)))
        plans.append(dict(field=field, k=flat_index(field, idx), lin=lin, rest=sp.Add(*rest)))
    return plans
