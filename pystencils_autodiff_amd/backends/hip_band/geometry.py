"""Eligibility, launch / LDS geometry and the (band height, rows per lane, depth) choice of the band schedule."""
import numpy as np

from ..hip_emitter import MarchConfig, zsum_plan


def band_plans(ir):
    """Per-store tap weights ``{(dz, dy, dx): coefficient}`` if the kernel fits the band schedule, else None."""
    if ir.ndim != 3 or ir.has_index_dims or ir.periodic:
        return None
    if len({np.dtype(f.dtype.numpy_dtype).itemsize for f in ir.fields}) != 1 or \
            np.dtype(ir.fields[0].dtype.numpy_dtype).itemsize not in (2, 4):
        return None                     # fp16 (fp32 arithmetic) or fp32 storage
    stencil = ir.stencil_fields
    if len(stencil) != 1 or any(r > 1 for r in ir.radius):
        return None
    if set(ir.fields) - set(ir.fields_written) - set(stencil):
        return None                     # other (point) fields read
    plans = zsum_plan(ir, MarchConfig(VE=8, ZSUM=True))
    if plans is None or not 1 <= len(plans) <= 2:
        return None
    out = []
    for pl in plans:
        if pl['rest'] != 0 or pl['k'] != 0:
            return None
        w = {}
        for dz, terms in pl['lin'].items():
            for coeff, f, dy, dx, k in terms:
                w[(dz, dy, dx)] = w.get((dz, dy, dx), 0) + coeff
        out.append(dict(field=pl['field'], w=w))
    return out


def band_esize(ir):
    return np.dtype(ir.fields[0].dtype.numpy_dtype).itemsize


def band_padded(X, es, pad):
    """Padded image rows (``BPAD``): rows of a 16-byte multiple only."""
    return bool(pad) and (X * es) % 16 == 0


def band_geometry(X, TY, R, D, es=2, pad=0, reg=0, free=0):
    """Launch / LDS geometry of a band of ``TY`` rows (``R`` per lane) on rows of ``X`` elements of ``es`` bytes.
    Rows whose pitch is not a multiple of 16 bytes (``X % VE``) take ``ceil(X / VE)`` chunks, the last one partial.
    ``pad``: every image row is preceded by one zero 16-byte piece and the slot ends with one (x neighbours of a row's
    end chunks read as zeros straight from LDS). ``reg``: rows of a partial last chunk on a padded image filled through
    registers (``BREG``). ``free``: the LDS handshake instead of plane barriers (``BFREE``), ``free - 1`` slots beyond
    ``D + 1``."""
    VE = 16 // es
    CPR = -(-X // VE)
    reg = bool(reg) and X % VE != 0
    padded = reg or band_padded(X, es, pad)
    # LDS image row pitch (elements, 16-byte multiple). Rows starting on half dwords (fp16, X odd) are loaded from the
    # dword at or below their start, one element early every other row: the image row then needs room for X + 2
    if padded:
        XP = (CPR + 1) * VE
    else:
        XP = CPR * VE if (X * es) % 4 == 0 else VE * -(-(X + 2) // VE)
    G = TY // R
    ntask = G * CPR
    NCT = -(-ntask // 64) * 64
    NPIECE = (TY + 2) * (XP // VE) + (1 if padded else 0)
    NI = -(-NPIECE // 64)
    SLOT = NI * 64 * VE
    NS = 3 if reg else D + 1 + max(0, int(free) - 1)
    return dict(VE=VE, CPR=CPR, XP=XP, G=G, ntask=ntask, NCT=NCT, NT=NCT + 64, NPIECE=NPIECE, NI=NI, SLOT=SLOT,
                NS=NS, lds_bytes=(NS * SLOT + 64) * es + (64 if free else 0), padded=padded, reg=reg)


def _fits(X, TY, R, D, es=2, pad=0, reg=0, idle=False, lds_kb=80):
    """Whether the geometry fits (compute lanes, the loader's vmcnt budget, ``lds_kb`` KB of LDS: 160 for the bands
    that take one workgroup per CU). Without ``idle`` every compute lane owns a task (``ntask`` a multiple of 64); with it the
    last compute wave may hold idle lanes."""
    g = band_geometry(X, TY, R, D, es, pad, reg)
    return (idle or g['ntask'] % 64 == 0) and g['NCT'] <= 960 and D * g['NI'] <= 63 and \
        g['lds_bytes'] <= lds_kb * 1024


def band_choice(X, nstore=1, es=2, pad=0, reg=0, idle=False, star=False, wide16=True):
    """(TY, R, D) for rows of X elements, or None. fp16, measured (scripts/probes/band_ab.py,
    profiles/r03_band_ab*.log): 8-row bands of 4 rows per lane with 2 planes in flight at X = 768 and 1024
    (27-point 1024³: 0.895 ms vs 0.921 for 4-row bands of 2 rows per lane, 3 planes in flight); three workgroups
    per CU. fp32 rows hold half the cells per 16-byte chunk: 4-row bands of 4 rows per lane first (the loader's
    vmcnt budget and 80 KB of LDS).

    Round 5 (profiles/r05_band_geo1.log, through the op, same process): fp16 rows of at least 96 chunks whose
    16-row band of 2 rows per lane fills whole compute waves (X = 768: 12 compute waves, one workgroup per CU)
    take that band first — 27-point 768³ fwd+bwd 0.675 vs 0.705-0.711 ms with 8-row bands of 4 rows (2 planes in
    flight; 18 rows read per 16 stored instead of 10 per 8: the memory pattern alone 0.640 vs 0.662 ms), fp16
    7-point 768³ 0.604 vs 0.630 (``star``: 1 plane in flight, 0.626 with 2). 512-wide rows (8 compute waves) keep the
    8-row bands (0.210 vs 0.198 ms); 1024-wide rows do not fit 16 row groups of 128 chunks."""
    VE = 16 // es
    if X < 16 * VE:
        return None
    rmax = 4 if nstore == 1 else 2
    CPR = -(-X // VE)
    if wide16 and es == 2 and CPR >= 96 and X % VE == 0:
        first = (16, 2, 1 if star else 2)
        # one workgroup per CU (up to 160 KB of LDS; the padded image at X = 768 takes 84 KB)
        if first[1] <= rmax and _fits(X, *first, es, pad, reg, lds_kb=160):
            return first
    # fp16: 16-row bands of 2 rows per lane before 4- / 8-row bands with 3 planes in flight (27-point 512²×640 0.279 vs
    # 0.335 ms, ×384 0.166 vs 0.170; fp16 7-point ×640 0.248 vs 0.252, ×384 0.149 vs 0.153: profiles/r04_op_band_823.log)
    cands = [(8, 4, 2), (16, 2, 2), (4, 2, 3), (8, 2, 3)] if es == 2 else [(4, 4, 2), (8, 4, 2), (4, 2, 2), (8, 2, 2)]
    cands += [(12, 4, 2), (16, 4, 2), (16, 2, 2), (32, 4, 2), (32, 2, 2)]
    for TY, R, D in cands:
        if R <= rmax and _fits(X, TY, R, D, es, pad, reg):
            return TY, R, D
    if idle:
        # rows whose chunk count leaves no band height of whole compute waves (X = 504 / 520 / 760 / 1000 halves: 63 /
        # 65 / 95 / 125 chunks): the last compute wave holds idle lanes. Measured through the op against the zsum
        # schedule these rows took before (profiles/r04_op_band_idle.log, fwd+bwd): 16-row bands of 2 rows per lane
        # first — 27-point 512²×520 0.246 vs 0.320 ms, ×504 0.217 vs 0.272, ×760 0.313 vs 0.400; fp16 7-point ×520
        # 0.194 vs 0.290, ×504 0.195 vs 0.249 — then 16-row bands of 4 rows per lane, one plane in flight (27-point
        # ×1000 0.402 vs 0.538). fp32: 8-row bands of 2 rows per lane (7-point ×520 0.389 vs 0.632 ms)
        order = [(16, 2, 2), (16, 4, 1), (8, 4, 2), (8, 2, 3)] if es == 2 else [(8, 2, 2), (8, 4, 2), (4, 4, 2)]
        for TY, R, D in order:
            if R <= rmax and _fits(X, TY, R, D, es, pad, reg, idle=True, lds_kb=160):
                return TY, R, D
    return None
