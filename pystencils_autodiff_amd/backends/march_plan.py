"""Which march kernel a launch gets: host code only, a pure function of the kernel IR, the field shape, pointer
alignment classes, tile overrides and the environment (no torch, no tensor, no device).

``default_march_config`` picks the tile (``MarchConfig``) of a kernel and field shape in stages — overrides, stencil
class, class defaults, override repairs, the row-band schedule (``_band_config``), fit to the shape, fit to the LDS,
the workgroup map. ``resolve_march`` adds what depends on one launch (the vector width and row-alignment route its
pointers allow, 32-bit plane offsets, border stores, band store masks, start signal, halo wait) and returns the final
``MarchConfig``, or None for the one-thread-per-cell schedule. ``tests/test_march_plan.py`` pins both. Periodic kernels
take their own, narrower path (``periodic_march_config``, ``_resolve_periodic``: LDS-DMA loader tiles on rows of whole
16-byte pieces only), pinned by ``tests/test_periodic_march.py``.

Environment: ``PSAD_MARCH="CX=..,NR=.."`` (tile overrides, ``_overrides``) and the switches read by ``_switch``:
``PSAD_BAND=0`` (no row-band schedule), ``PSAD_BAND_UNALIGNED=0`` (none on rows of other pitches than 16 bytes),
``PSAD_XO=0`` (no half-dword rows on the half-precision LDS-DMA ring).
"""
import math
import os
from dataclasses import replace
from types import SimpleNamespace

import numpy as np

from .hip_band import band_choice, band_esize, band_geometry, band_plans
from .hip_emitter import (MarchConfig, lite_fields, march_geometry, ncomp, pair_ok, storage_ctype, ws_geometry,
                          zsum_plan)

# row-band defaults, settled A/B rounds through the op (fn.apply + backward, same process;
# scripts/probes/op_band_ab.py, profiles/r03_op_band_ab*.log): box stencils (27 taps) 48-plane chunks without the
# trimmed chunk-edge planes (fwd+bwd 1024³ 1.707 vs 1.809 ms zsum, trimmed 24-plane chunks 2.01; 768³ 0.731 vs
# 0.762), star stencils 8-plane chunks (fp16 7-point 1024³ 1.461 vs 1.538, 768³ 0.635 vs 0.682). Launches of fewer
# than BAND_MIN_WG workgroups (z-slabs of a few planes) keep the zsum ring.
BAND_ZC_BOX, BAND_ZC_STAR = 48, 8
# round 4 (profiles/r04_op_band_ab1.log, same process, fwd+bwd through the op): the chunk's first two planes peeled
# without the taps of outputs before it (BTRIM=1) — 27-point 768³ 0.744 vs 0.768 ms, 1024³ 16-row bands 1.718 vs 1.744
# (and 1.679 with 32-plane chunks), fp16 7-point 768³ 0.602 vs 0.626
BAND_ZC_BOX16 = 32
# round 4 (profiles/r04_op_band_ab3.log .. _ab5.log): both chunk ends peeled at a compile-time chunk length (BTRIM=3)
# — 27-point 768³ 0.715 vs 0.724 ms (BTRIM=1), 1024³ 1.617 vs 1.640, fp16 7-point 768³ 0.594 vs 0.595-0.633
BAND_TRIM_DEFAULT = 3
# box-stencil chunk length: the longest of BAND_ZC_BOX_LADDER that still gives BAND_ROUND_WG workgroups (one
# round of three per CU; profiles/r04_op_zc_sweep.log): 27-point 512³ 32 planes 0.209 ms vs 16 0.243, 8 0.235;
# 256³ 8 planes 0.028 vs 11 0.036, 16 0.045; a 96×768² slab 12 planes 0.091 vs 8 0.095, 24 0.109
BAND_ZC_BOX_LADDER = (48, 32, 24, 16, 12, 8)
BAND_ROUND_WG = 768
BAND_MIN_WG = 768
# star stencils: 8-plane chunks, but 64-plane chunks on rows of <= 512 elements when that still gives >= 512
# workgroups (profiles/r04_op_zc_sweep.log, _ab6.log): fp16 7-point 512³ 0.184 vs 0.197 ms, 510³ 0.204 vs 0.229;
# 768³ keeps 8 (0.629 vs 0.675 at 96 planes, 0.699 at 64), 256³ too (0.024 vs 0.038 at 32)
BAND_ZC_STAR_LONG, BAND_STAR_LONG_MAX_X, BAND_STAR_LONG_MIN_WG = 64, 512, 512
# fp32 storage (4 cells per 16-byte chunk): 4-row bands measured slower through the op (7-point 512³ 0.387 vs
# 0.373 ms, 768³ 1.325 vs 1.261); 8-row bands of 4 rows per lane (4 compute waves, 60 KB of LDS) faster for star
# stencils on rows of <= 512 on every box (profiles/r04_op_f7_ab2.log .. _ab4.log, shared inputs): 512³
# 0.365-0.368 vs 0.373-0.389 ms; at 768 (6 compute waves, one workgroup per CU) it won on one box (1.189 vs 1.219)
# and lost on another (1.283-1.318 vs 1.261): zsum there. Box stencils in fp32 stay on zsum unless BAND=R asks.
BAND_F32_STAR_MAX_X = 512
BAND_ZC_STAR_F32 = 16
# zero-padded image rows (x neighbours read from LDS, no DPP / boundary selects) for box stencils
# (profiles/r04_op_band_ab6.log): 27-point 768³ 0.699 vs 0.715 ms, 1024³ 1.581 vs 1.603, 512³ 0.198 vs 0.201;
# fp16 7-point 768³ 0.631 vs 0.629, 1024³ 1.444 vs 1.438 (not for star stencils)
BAND_PAD_BOX = 1
# partial rows on a padded image filled through registers (BREG) for star stencils on fp16 rows of odd length
# (profiles/r04_op_band_ab9.log): 7-point 511³ 0.210 vs 0.217 ms (DMA row pieces + v_perm realignment); even rows
# (510³ 0.207 vs 0.201) and box stencils (27-point 510³ 0.259 vs 0.245, 511³ 0.259 vs 0.252) keep the DMA pieces
BAND_REG_STAR_ODD = 1
# fp32 star stencils on rows with no whole-wave band height (idle lanes, hip_band.band_choice): the band up to this
# row length (7-point 512²×520 0.389 vs 0.632 ms on zsum, profiles/r04_op_band_idle.log)
BAND_F32_IDLE_MAX_X = 1024

# (CX, NR) candidates of the LDS-DMA plane ring for stencils that are not linear off the centre plane
# (hip_emitter.geometry._ring_ws_geometry), widest first: the first whose ring fits the LDS
RING_WS_TILES = ((4, 4), (4, 2), (2, 4), (2, 2), (1, 4), (1, 2), (1, 1))

# gpu_indexing_params keys of pystencils' own GPU indexing (``block_size``, ``maximum_block_size``, …, e.g.
# ``gpu_indexing_params={'block_size': (8, 4, 2)}`` in the reference's tests/test_graph_datahandling.py:70): they
# describe a one-thread-per-cell launch these schedules do not have, so they are accepted and ignored. Upper-case
# keys are this layer's tile parameters; an unknown one is a typo and raises.
TILE_KEYS = ('CX', 'WX', 'NR', 'ZMIN', 'ZMAX', 'BLK', 'D', 'NW', 'NT_STORE', 'ZSUM', 'PK', 'WS', 'AR', 'VIEW2D', 'ZC',
             'BLOCKS', 'MAP', 'BAND', 'BTY', 'BTRIM', 'BEDGE', 'BPAD', 'BZF', 'BREG', 'BNT', 'BFREE', 'BTAIL',
             'SFAST', 'SLP', 'PR', 'PD')
# the tile keys that are MarchConfig fields of the zsum / ring schedules, by type (the others: the chunk target of
# ``march_launch_geometry`` and the band keys, which ``_band_config`` reads)
KEY_TYPES = {**dict.fromkeys(('CX', 'WX', 'NR', 'ZMIN', 'ZMAX', 'BLK', 'D', 'NW', 'MAP', 'SFAST', 'SLP', 'PR', 'PD'), int),
             **dict.fromkeys(('NT_STORE', 'ZSUM', 'PK', 'WS', 'AR'), lambda v: v if isinstance(v, bool) else bool(int(v))),
             'VIEW2D': str}
# Ablation knobs that make results WRONG (timing probes: ``BABL``). They are not tile keys — ``gpu_indexing_params`` and
# ``PSAD_MARCH`` reject them — and reach the planner only through this dict, which nothing on the op's path writes:
# a probe script sets it explicitly (``scripts/probes/op_band_ab.py``) and clears it again.
PROBE_KEYS = ('BABL',)
PROBE_KNOBS = {}

LDS_MAX = 160 * 1024
# the planes the LDS-DMA loaders and the band kernels address with 32-bit byte offsets
OFFSET_MAX = 2 ** 31 - 1024


def _switch(name):
    return os.environ.get(name, '1') != '0'


def _ladder_chunk(nty, Z):
    return next((c for c in BAND_ZC_BOX_LADDER if nty * -(-Z // c) >= BAND_ROUND_WG), BAND_ZC_BOX_LADDER[-1])


# ---------------------------------------------------------------------------------------------- the row-band schedule
def _band_applies(ir, shape, over):
    """The band is asked for at all: the row length is known and no tile override asks for another schedule
    (``BAND=0`` or ``PSAD_BAND=0`` turn it off, ``BAND=R`` turns it on)."""
    if shape is None or ir.ndim != 3 or not _switch('PSAD_BAND'):
        return False
    if 'BAND' in over:
        return bool(int(over['BAND']))
    return not any(k in over for k in ('CX', 'WX', 'NR', 'NW', 'ZSUM', 'PK', 'WS', 'AR', 'VIEW2D'))


def _band_tile(shape, nplans, es, star, over):
    """``(TY, R, D, pad, reg, rule16)`` — band height, rows per lane, planes in flight, image layout, and whether the
    1024-wide box rule chose it — or None where the band is not the default for these rows."""
    Z, Y, X = (int(n) for n in shape)
    forced = 'BAND' in over
    whole = band_choice(X, nplans, es, star=star)
    if whole is not None and whole[:2] == (16, 2) and not forced:
        # the wide-row 16-row band (one workgroup per CU) only where its launch still fills three rounds of the
        # chip with the chunk length it would take (a 96×768² slab would get 576 workgroups: 8-row bands there)
        nty16 = -(-Y // 16)
        zc16 = BAND_ZC_STAR if star else _ladder_chunk(nty16, Z)
        if nty16 * -(-Z // zc16) < BAND_ROUND_WG:
            whole = band_choice(X, nplans, es, star=star, wide16=False)
    if es == 4 and not forced and not (star and X <= (BAND_F32_STAR_MAX_X if whole else BAND_F32_IDLE_MAX_X)):
        return None
    # rows with no band height of whole compute waves: a band whose last compute wave holds idle lanes
    choice = whole or band_choice(X, nplans, es, idle=True)
    if choice is None:
        return None
    TY, R, D = choice
    pad = int(over.get('BPAD', 0 if star else BAND_PAD_BOX))
    reg = int(over.get('BREG', BAND_REG_STAR_ODD if star and es == 2 and X % 2 and not int(over.get('BFREE', 0))
                       else 0))                 # (the LDS handshake takes the LDS-DMA loader)
    # fp32 star stencils: 8-row bands of 4 rows per lane (see BAND_F32_STAR_MAX_X) — one output only (band_choice's
    # rule: at most 2 rows per lane when a kernel stores two fields)
    g8 = band_geometry(X, 8, 4, 2, 4, pad, reg) if es == 4 and nplans == 1 else None
    if g8 and star and not forced and g8['ntask'] % 64 == 0 and g8['NCT'] <= 960 and \
            2 * g8['NI'] <= 63 and g8['lds_bytes'] <= LDS_MAX:
        TY, R, D = 8, 4, 2
    zc0 = int(over.get('ZMIN', BAND_ZC_STAR if star else BAND_ZC_BOX))
    rule16 = not star and es == 2 and (X // 8) % 128 == 0 and R == 4 and -(-Y // 16) * -(-Z // zc0) >= BAND_MIN_WG
    if rule16:
        # box stencils on rows of a multiple of 1024 halves: 16-row bands, one plane in flight (18/16 rows read per
        # band instead of 10/8; 72 KB LDS): 27-point 1024³ fwd+bwd 1.712-1.719 vs 1.764-1.766 ms with 8-row bands
        # (profiles/r03_op_band_ab5.log, _ab6.log); the 7-point star stencil loses (1.65 vs 1.42), 768-wide rows too
        TY, D = 16, 1
    if forced:
        R = int(over['BAND'])
    TY = int(over.get('BTY', TY if TY % R == 0 else R * max(1, TY // R)))
    return TY, R, int(over.get('D', D)), pad, reg, rule16


def _band_chunk(shape, TY, es, star, rule16):
    """``(chunk length, minimum workgroup count)`` of a band of ``TY`` rows."""
    Z, Y, X = (int(n) for n in shape)
    nty = -(-Y // TY)
    if star and es == 4:
        return BAND_ZC_STAR_F32, BAND_MIN_WG
    if star:
        long_ok = X <= BAND_STAR_LONG_MAX_X and nty * -(-Z // BAND_ZC_STAR_LONG) >= BAND_STAR_LONG_MIN_WG
        return (BAND_ZC_STAR_LONG, BAND_STAR_LONG_MIN_WG) if long_ok else (BAND_ZC_STAR, BAND_MIN_WG)
    if TY == 16 and rule16:
        return BAND_ZC_BOX16, BAND_MIN_WG   # (16-row bands of other rows — 2 rows per lane, idle lanes — take the ladder)
    return _ladder_chunk(nty, Z), BAND_MIN_WG


def _band_config(ir, ve, shape, over):
    """The row-band schedule (``hip_band``) for the stencils it fits — fp16 storage, and fp32 star stencils on rows of
    up to ``BAND_F32_STAR_MAX_X`` / ``BAND_F32_IDLE_MAX_X`` elements — when the row length is known and no tile
    override asks for another schedule (``BAND=0`` or ``PSAD_BAND=0`` turn it off, ``BAND=R`` / ``BTY`` pick
    rows per lane / band height)."""
    plans = band_plans(ir) if _band_applies(ir, shape, over) else None
    if not plans:
        return None
    es, star, X = band_esize(ir), max(len(pl['w']) for pl in plans) <= 12, int(shape[-1])
    tile = _band_tile(shape, len(plans), es, star, over)
    if tile is None:
        return None
    TY, R, D, pad, reg, rule16 = tile
    free = int(over.get('BFREE', 0))
    g = band_geometry(X, TY, R, D, es, pad, reg, free=free)
    if TY % R or g['NCT'] > 960 or D * g['NI'] > 63 or g['lds_bytes'] > LDS_MAX or g['NT'] > 1024:
        raise ValueError(f'band schedule: BTY={TY} BAND={R} D={D} do not fit rows of {X} elements')
    zc, min_wg = _band_chunk(shape, TY, es, star, rule16)
    zc = int(over.get('ZMIN', zc))
    if 'BAND' not in over and -(-int(shape[-2]) // TY) * -(-int(shape[0]) // zc) < min_wg:
        return None
    zmax = int(over.get('ZMAX', zc))
    btrim = int(over.get('BTRIM', BAND_TRIM_DEFAULT))
    if btrim == 3 and (zmax != zc or zc < 3):
        if 'BTRIM' in over:
            raise ValueError('band schedule: BTRIM=3 needs ZMIN == ZMAX >= 3')
        btrim = 1                       # chunk length not fixed at compile time: peel the chunk's first planes only
    return MarchConfig(VE=ve, BAND=R, BTY=TY, BX=X, D=D, ZSUM=True, NT_STORE=True, ZMIN=zc,
                       ZMAX=zmax, BLK=int(over.get('BLK', 512)), MAP=int(over.get('MAP', 0)),
                       BTRIM=btrim, BEDGE=int(over.get('BEDGE', 1)), BPAD=pad, BZF=int(over.get('BZF', 1)), BREG=reg,
                       BNT=int(over.get('BNT', 2)), BFREE=free, BTAIL=int(over.get('BTAIL', 1)),
                       BABL=int(PROBE_KNOBS.get('BABL', 0)))


# ------------------------------------------------------------------------------------------------ the tile, in stages
def _overrides(tuning):
    """Stage 1: the tile overrides of ``gpu_indexing_params`` (upper-case keys; pystencils' own indexing keys are
    ignored) and ``PSAD_MARCH``, which wins; unknown keys raise, values take their type."""
    over = {k: v for k, v in dict(tuning or {}).items() if not k.islower()}
    env = os.environ.get('PSAD_MARCH')
    for kv in env.split(',') if env else ():
        k, v = kv.split('=')
        over[k.strip()] = v.strip() if k.strip() == 'VIEW2D' else int(v)
    for k, v in over.items():
        if k not in TILE_KEYS:
            raise ValueError(f"unknown tile parameter '{k}' (gpu_indexing_params / PSAD_MARCH)")
        over[k] = KEY_TYPES.get(k, lambda v: v)(v)
    return over


BASE = dict(CX=4, WX=1, NR=8, NT_STORE=True, VIEW2D='yx', ZSUM=False, PK=False, ZMIN=32, ZMAX=64, BLK=512)


def _stencil_class(ir, ve):
    """Stage 2: what the defaults need to know of ``(ir, ve)`` — ``linear`` off the centre plane (the zsum schedule
    applies), ``plane2d`` (2-D with no remainder beside the centre-plane sum), ``box`` (fields read off-centre behind
    the centre plane: no lite ring), ``half`` (fp16 storage), ``wide`` (fp64 arithmetic). (``pair_ok``, which only
    nonlinear kernels are asked, stays with the rules that ask it.)"""
    probe = MarchConfig(VE=ve, **BASE)
    plans = zsum_plan(ir, probe)
    linear = plans is not None
    return SimpleNamespace(linear=linear, plane2d=linear and all(pl['rest'] == 0 for pl in plans),
                           box=bool(set(ir.stencil_fields) - lite_fields(ir, probe)),
                           half=any(storage_ctype(f) == '_Float16' for f in ir.stencil_fields),
                           wide=np.dtype(ir.compute_dtype).itemsize == 8)


def _linear_3d(ir, ve, sc):
    """Stage 3, 3-D stencils linear off the centre plane: ``(cfg, ring)``, ring = 'star' on the star LDS-DMA ring."""
    cfg = dict(BASE)
    if sc.box:           # box stencil linear off-centre (27-point): z partial sums, small tile, short chunks
        # 768³ fp16: 0.460 ms (packed fp32 FMAs over column pairs, 2 waves side by side in x)
        # vs 0.469 scalar WX=1 vs 0.70 ms LDS ring; unrolling the plane loop 3x is slower (0.53-0.56)
        # chunks of 16..32 planes, ~2048 workgroups: 768³ 32 planes; one 8-GPU slab (96×768²) 16
        # planes, 0.067 vs 0.073 ms at 32
        # tap pairs by inline-asm ds_read2_b32 (AR): 0.421 vs 0.459 ms at 768³, 0.062 vs 0.067 ms per
        # 8-GPU slab (profiles/r01_tune_27pt_ar.log) — the compiler's adjacent-x merges cost 26 v_mov
        cfg.update(CX=2, WX=2, NR=4, ZSUM=True, PK=True, AR=True, ZMIN=16, ZMAX=32, BLK=2048)
        half = dict(CX=4, WX=1, NR=2, WS=True, D=3, ZMIN=24, ZMAX=24)
        if ws_geometry(ir, MarchConfig(VE=ve, **{**cfg, **half})):
            # fp16 storage: LDS-DMA loader wave into a half-precision ring, lanes own x-adjacent quads,
            # taps converted in registers (emit_zsum -> _emit_zsum_half), 256×8 tiles, 24-plane chunks:
            # 768³ 0.370-0.392 ms vs 0.431-0.448 ms for the register-prefetch AR form in the same
            # process; 96×768² slab 0.048-0.055 vs 0.059-0.069 ms (profiles/r02_tune_27pt_half*.log)
            cfg.update(half)
        return cfg, None
    cfg.update(ZSUM=True)                                  # 1024³ 7-point: 1.495 ms vs 1.629 ms lite ring
    ws0 = ws_geometry(ir, MarchConfig(VE=ve, **{**cfg, 'WS': True}))
    if not ws0:
        return cfg, None
    # star stencils, storage = compute type: LDS-DMA loader wave, 4 planes in flight, 256×16 tiles,
    # 128-plane chunks (one 5-wave workgroup per CU). 1024³ 7-point 1.411 ms vs 1.506 ms register
    # prefetch (128×32 tiles); one 8-GPU slab 0.182 vs 0.187 ms (profiles/r01_tune_ws_*.log).
    # fp16 storage (half-precision ring): 256×32 tiles, the same 16 KB per plane and workgroup:
    # 7-point fp16 1024³ 0.786 vs 0.889 ms, 768³ 0.372 vs 0.405, 128×1024² slab 0.092 vs 0.098,
    # 512³ 0.086 vs 0.087 (profiles/r02_tune_f16s_*.log). Chunks down to 8 planes: small domains are
    # latency bound with few long chunks (128³ 0.0106 vs 0.0197-0.021 ms, 256³ 0.0244 vs 0.032-0.036;
    # the chunk model keeps 1024³ / 768³ / 512³ / the 8-GPU slabs where they were,
    # profiles/r02_tune_small_*.log)
    cfg.update(WS=True, CX=4, NR=8 if ws0['kind'] == 'h' else 4, D=4, ZMIN=8, ZMAX=128, BLK=256)
    return cfg, 'star'


def _ring_3d(ir, ve, sc):
    """Stage 3, 3-D stencils not linear off the centre plane (products / functions of neighbour taps): the plane ring
    fed by an LDS-DMA loader wave, 2 planes in flight, the widest tile whose ring fits the LDS (ring = 'ring'), else
    the register-prefetch ring."""
    cfg, tiles = dict(BASE), RING_WS_TILES
    if sc.half and pair_ok(ir):
        # fp16 planes in the ring, taps as whole dwords of cell pairs (PR): 128×8 tiles, two planes in flight, for
        # two ring fields (varcoef forward), 128×4 and three in flight for more (its adjoint: three fields). 768³
        # fwd / bwd 0.618–0.634 / 1.066–1.095 ms vs 0.67–0.69 / 1.16–1.17 on the register ring
        # (profiles/r06_hring_f16.log, r06_hring_f16b.log: 20 tilings, 8 compute waves and deeper rings slower)
        tiles = [(2, 2 if len(ir.stencil_fields) <= 2 else 1)]
        cfg['PR'] = 1
    half_vec = ir.has_index_dims and sc.half
    if half_vec:
        # vector fields in fp16 (fp16 images, taps converted): 128×8 tiles. Lanes own x-adjacent cell pairs with
        # packed fp32 statements (PR) where the statements allow — a lane's elements are then contiguous from an
        # even offset and its reads merge; eight compute waves for the adjoint's two ring fields. Advection u(3)
        # 256³ fwd / bwd 0.052 / 0.054 ms vs 0.063 / 0.063 per cell, 0.139 / 0.069 on the widest fitting tile
        # (256×16), 0.131 / 0.153 one thread per cell (profiles/r06_vec16_tiles.log, r06_vec16_pairs.log; fp32
        # vector fields measured slower as pairs: 0.075 / 0.12 vs 0.071 / 0.095)
        tiles = [(2, 2)]
        if pair_ok(ir, vectors=True):
            cfg['PR'] = 1
    for cx, nr in tiles:
        c = {**cfg, 'CX': cx, 'NR': nr, 'WS': True, 'D': 2 if nr == 2 or not cfg.get('PR') else 3, 'ZMIN': 8,
             'ZMAX': 128, 'BLK': 256}
        if half_vec and len(ir.stencil_fields) > 1:
            c['NW'] = 8
        w = ws_geometry(ir, MarchConfig(VE=ve, **c))
        if w is not None and w['lds_bytes'] <= LDS_MAX:
            return c, 'ring'
    cfg['PR'] = 0                 # (the register ring stores fp32 images: pairs measured neutral there)
    # nonlinear stencils on the register-prefetch ring (fp16 storage: the LDS-DMA ring holds the compute type):
    # 128×8 tiles, four workgroups per CU — varcoef fp16 768³ fwd / bwd 0.69–0.71 / 1.16–1.18 ms vs 0.81 / 1.31–1.34
    # with the budget's 256×16 / 256×8 (profiles/r06_varcoef_f16_tiles.log: latency, not VALU — packed cell pairs
    # or two planes in flight on the wide tiles gave nothing, r06_varcoef_pairs_f16.log, r06_varcoef_pd2_f16.log)
    cfg.update(CX=2, NR=2)
    return cfg, None


def _defaults_2d(ir, ve, sc, shape):
    """Stage 3, 2-D fields: (1, Y, X) tiles, or for nonlinear stencils on long rows the row ring (ring = 'ring')."""
    cfg = {**BASE, 'NR': 4, 'NT_STORE': False}                  # 256×16 tiles (4096²: 0.024 ms, 5.6 TB/s)
    if sc.plane2d:
        return cfg, None
    # nonlinear 2-D stencils (one tile per workgroup, nothing to pipeline): 128×8 tiles, more workgroups in
    # flight — 2-D varcoef 4096² fp32 fwd / bwd 0.52 / 0.51 of 8 TB/s vs 0.49 / 0.38 on 256×16, fp16 0.30 /
    # 0.35 vs 0.28 / 0.21 (profiles/r06_nl2d.log)
    cfg.update(CX=2, NR=2)
    # ... and on long 16-byte-piece rows: march along axis 0 (VIEW2D='zy', rows as the planes of the LDS-DMA
    # ring, four waves side by side in x: 512-cell row strips; fp16 as x-adjacent cell pairs), 512 / 1024
    # workgroups of 64 / 32 rows at 4096²: 2-D varcoef 4096² fp32 fwd / bwd 0.61 / 0.57–0.58 of 8 TB/s,
    # fp16 0.40–0.42 / 0.49 (profiles/r06_nl2d_zy.log: 40 tilings and chunkings; the register ring along
    # axis 0 was slower, 0.41 / 0.41, and 128-row chunks 0.51 / 0.49)
    # (fp64: 1024-cell strips, not halved below — fwd / bwd 0.56–0.62 / 0.58–0.61 vs 0.55–0.56 / 0.53–0.56 on
    # the (1, Y, X) tiles; 256-cell strips lost the adjoint, 0.53, profiles/r06_nl2d_f64.log)
    zy = dict(VIEW2D='zy', NR=1, NW=4, WX=4, CX=4 if sc.wide else 2, WS=True, D=2, ZMIN=16 if sc.half else 32,
              ZMAX=64, BLK=1024 if sc.half else 512, PR=1 if sc.half and pair_ok(ir, vectors=True) else 0)
    if ir.stencil_fields and (shape is None or int(shape[-1]) >= 64 * zy['CX'] * zy['WX']):
        w = ws_geometry(ir, MarchConfig(VE=ve, **{**cfg, **zy}))
        if w is not None and w['lds_bytes'] <= LDS_MAX:
            return {**cfg, **zy}, 'ring'
    return cfg, None


def _class_defaults(ir, ve, sc, shape):
    """Stage 3: the measured tile of the stencil's class as a ``MarchConfig`` field dict, and the LDS-DMA ring it
    took: 'star' (star stencils on the zsum schedule), 'ring' (the plane ring of nonlinear stencils, 3-D or 2-D along
    axis 0) or None."""
    cfg, ring = dict(BASE), None
    if ir.ndim == 3:
        cfg, ring = (_linear_3d if sc.linear else _ring_3d)(ir, ve, sc)
    elif ir.ndim == 2:
        cfg, ring = _defaults_2d(ir, ve, sc, shape)
    if ir.has_index_dims and ring != 'ring':
        # vector fields (components interleaved in the plane image) linear off the centre plane: the zsum schedule;
        # narrower tiles keep the image (TX + 2H)·C elements wide (the plane ring picked its tile above)
        cfg.update(ZSUM=True, PK=False, AR=False)
        while cfg['CX'] > 1 and cfg['CX'] * max([ncomp(f) for f in ir.stencil_fields] + [1]) > 4:
            cfg['CX'] //= 2
    if sc.wide and not (ir.ndim == 2 and ring == 'ring'):
        cfg['CX'] = max(1, cfg['CX'] // 2)                     # fp64: half-width tiles (512³: 0.380 vs 0.536 ms)
    elif ir.ndim == 3 and cfg['ZSUM'] and not cfg['PK'] and not cfg.get('WS'):
        # star stencils: 128×32 tiles, two workgroups per CU. 512³ / one 8-GPU slab of 1024³
        # (128×1024²): 0.191 / 0.187 ms vs 0.214 / 0.208 ms with 256×32 tiles; 1024³ a tie
        cfg['CX'] = 2
    return cfg, ring


def _apply_overrides(ir, ve, sc, cfg, ring, over):
    """Stage 4: the overrides on the class defaults — first the repairs of defaults an override cannot combine with."""
    view_yx = ir.ndim == 2 and str(over.get('VIEW2D', cfg['VIEW2D'])) != cfg['VIEW2D']
    if ring == 'ring' and (any(k in over for k in ('CX', 'WX', 'NR', 'NW')) or view_yx) and 'WS' not in over:
        cfg.update(WS=False, D=3)           # a tile override on the ring: the register-prefetch form it was sized for
        if ir.ndim == 2:
            cfg.update(VIEW2D='yx', NW=4, WX=1, NR=2, PR=0, ZMIN=32, ZMAX=64, BLK=512,   # (the 2-D one: (1, Y, X) tiles)
                       CX=1 if sc.wide else 2)
            if ir.has_index_dims:
                cfg.update(ZSUM=True, PK=False, AR=False)     # (vector fields: the zsum plane, as without the ring)
            ring = None
    cfg.update({k: v for k, v in over.items() if k in KEY_TYPES})
    if cfg.get('PR') and 'PR' not in over and (cfg['CX'] % 2 or not pair_ok(ir, vectors=bool(cfg.get('WS')))):
        cfg['PR'] = 0          # a tile override the default pair form cannot take (odd CX; vector fields off the ring)
    if ring == 'ring' and PROBE_KNOBS.get('BABL'):
        cfg['BABL'] = int(PROBE_KNOBS['BABL'])   # (timing probe of the march ring, as on the band: 3 = no plane loads)
    if 'NW' in over and 'WX' not in over:
        cfg['WX'] = min(cfg['WX'], cfg['NW'])
    if cfg['ZSUM'] and zsum_plan(ir, MarchConfig(VE=ve, **cfg)) is None:
        cfg['ZSUM'] = False                                    # not eligible: LDS ring instead
    return cfg


def _fit_shape(ir, ve, cfg, over, shape, cmin):
    """Stage 6: tiles no wider / taller than the field needs (overridden keys stay)."""
    X = int(shape[-1])
    if 'CX' not in over:
        while cfg['CX'] > cmin and 64 * cfg['CX'] * cfg['WX'] // 2 >= X:
            cfg['CX'] //= 2
        tx = 64 * cfg['CX'] * cfg['WX']
        ws0 = ws_geometry(ir, MarchConfig(VE=ve, **cfg)) if cfg.get('WS') else None
        quads = ws0 is not None and ws0['kind'] == 'h'       # the half ring needs lanes owning quads
        if cfg.get('WS') and cfg['CX'] > cmin and -(-X // (tx // 2)) * (tx // 2) < -(-X // tx) * tx and \
                (not quads or (cfg['CX'] // 2) % 4 == 0):
            # WS tiles: half width when it pads x less (384³ 7-point: 0.116 → 0.081 ms with 48-plane
            # chunks, profiles/r01_tune_odd_sizes.log)
            cfg['CX'] //= 2
    if 'WX' not in over:
        while cfg['WX'] > 1 and 64 * cfg['CX'] * cfg['WX'] // 2 >= X:
            cfg['WX'] //= 2
    ny = int(shape[-2]) if ir.ndim == 3 or cfg['VIEW2D'] == 'yx' else 1
    if 'NR' not in over:
        while cfg['NR'] > 1 and (cfg.get('NW', 4) // cfg['WX']) * cfg['NR'] // 2 >= ny:
            cfg['NR'] //= 2


def _lds(ir, ve, cfg):
    mc = MarchConfig(VE=ve, **cfg)
    return (ws_geometry(ir, mc) or march_geometry(ir, mc))['lds_bytes']


def _drop_loader(c):
    """The register-prefetch form of an LDS-DMA loader config (a ``MarchConfig`` field dict): eight compute waves
    exist only on the LDS-DMA ring, so NW drops to 4 (and WX to at most 4)."""
    c['WS'] = False
    if c.get('NW', 4) == 8:
        c['NW'], c['WX'] = 4, min(c['WX'], 4)
    return c


def ws_fallback_config(cfg):
    """The register-prefetch form of a WS (LDS-DMA loader) config, for planes beyond the loader's 32-bit buffer
    offsets (``_drop_loader``, as in ``default_march_config``'s own fallback)."""
    return MarchConfig(**_drop_loader(dict(cfg.__dict__)))


def _fit_lds(ir, ve, cfg, over, cmin):
    """Stage 7. LDS budget: two workgroups per CU (≤ 80 KB) for the register-prefetch defaults, the 160 KB hardware
    limit for the LDS-DMA ring and for explicit tile overrides."""
    budget = 80 * 1024 if not ('CX' in over or 'NR' in over or cfg.get('WS')) else LDS_MAX
    while cfg.get('WS') and cfg.get('D', 3) > 1 and _lds(ir, ve, cfg) > LDS_MAX:
        cfg['D'] = cfg.get('D', 3) - 1                          # fewer planes in flight before smaller tiles
    while _lds(ir, ve, cfg) > budget and (cfg['NR'] > 1 or cfg['CX'] > cmin):
        if (cfg['NR'] >= cfg['CX'] or cfg['CX'] <= cmin) and cfg['NR'] > 1:
            cfg['NR'] //= 2
        else:
            cfg['CX'] //= 2
    if cfg.get('WS') and not cfg['ZSUM'] and _lds(ir, ve, cfg) > LDS_MAX:
        # a plane ring that does not fit even at the smallest tile (many fields of wide radius): the register form
        # (of that smallest tile: the halving above stopped at it)
        _drop_loader(cfg)
    if ir.ndim == 3 and _lds(ir, ve, cfg) > LDS_MAX:
        raise ValueError(f'no tile of this kernel fits the 160 KB LDS ({_lds(ir, ve, cfg)} B at {cfg})')


def default_march_config(ir, ve, shape=None, tuning=None, band=True):
    """Tile shape for a kernel and field shape (measured on MI355X).

    3-D stencils linear in their off-centre planes use the z-partial-sum schedule (``emit_zsum``):
    star stencils (7-point) with a 256×32 tile (CX=4, NR=8), box stencils (27-point) with a
    128×16 tile and 32-plane chunks; fp64 halves the tile width (register pressure). Other 3-D
    stencils use the LDS ring ("lite" ring when planes behind the centre are read only at (0,0)).
    2-D fields run as (1, Y, X) tiles of 256×16. Non-temporal stores for 3-D outputs (written
    once, never re-read by the sweep). Overrides: ``gpu_indexing_params`` or
    ``PSAD_MARCH="CX=..,NR=.."``. With ``band`` the row-band schedule (``_band_config``) goes first.
    """
    over = _overrides(tuning)
    bc = _band_config(ir, ve, shape, over) if band else None        # stage 5, which needs the overrides alone
    if bc is not None:
        return bc
    sc = _stencil_class(ir, ve)
    cfg, ring = _class_defaults(ir, ve, sc, shape)
    cfg = _apply_overrides(ir, ve, sc, cfg, ring, over)
    cmin = 2 if cfg.get('PR') and not cfg['ZSUM'] else 1      # packed cell pairs: two cells per lane and column
    if shape is not None:
        _fit_shape(ir, ve, cfg, over, shape, cmin)
    _fit_lds(ir, ve, cfg, over, cmin)
    if ring == 'star' and cfg.get('WS') and shape is not None and 'MAP' not in over:
        ntx = -(-int(shape[-1]) // (64 * cfg['CX'] * cfg['WX']))
        if ntx & (ntx - 1):
            # tiles per row not a power of two: dispatch order instead of the XCD-aware remap. Through the op,
            # fwd + bwd, same process (scripts/probes/map_ab.py, profiles/r03_map_ab.log): 768³ fp32 -8.6 %
            # (5.91 / 5.78 TB/s), 640³ -4.4 %, 768³ fp16 -4.7 %, 640³ fp64 -2.5 %; with 2 or 4 tiles per row
            # the dispatch order pins each XCD to the same x columns of every plane: 1024³ +10 %, 128×1024²
            # +10 %, 512³ fp64 +6 % — those keep the remap
            cfg['MAP'] = 1
    return MarchConfig(VE=ve, **cfg)


# ---------------------------------------------------------------------------------------------------- one launch
def align_class(p):
    """log2 of the largest power of two (≤ 32) dividing the address ``p`` (0 counts as 32-byte aligned)."""
    return min((p & -p).bit_length() - 1, 5) if p else 5


def is_pair(z_range):
    return len(z_range) == 2 and all(isinstance(r, (tuple, list)) for r in z_range)


def march_extents(ir, shape, cfg, z_range=None, z_limits=None):
    """(Z, Y, X), the iteration bounds (``z_limits`` replacing, ``z_range`` restricting those of axis 0; a pair of
    ranges is checked and spans from its first plane to its last) and the tiles per row and column of the march
    schedule for a field shape."""
    bounds = ir.iteration_bounds(shape)
    if z_limits is not None:
        bounds[0] = (int(z_limits[0]), int(z_limits[1]))
    if z_range is not None:
        if ir.ndim == 2 and cfg.VIEW2D == 'yx':
            raise ValueError("z ranges need the 'zy' view of 2-D fields")
        lo, hi = bounds[0]
        if is_pair(z_range):
            (a0, a1), (b0, b1) = [(int(a), int(b)) for a, b in z_range]
            if not (lo <= a0 < a1 <= b0 < b1 <= hi) or a1 - a0 != b1 - b0:
                raise ValueError(f'z_range pair {z_range} must be disjoint, ordered, of equal length '
                                 f'and inside [{lo}, {hi})')
            z_range = (a0, b1)
        bounds[0] = (max(lo, int(z_range[0])), min(hi, int(z_range[1])))
    if ir.ndim == 2:        # one plane of (1, Y, X) tiles, or rows as the planes of a march along axis 0: (Y, 1, X)
        axis = 0 if cfg.VIEW2D == 'yx' else 1
        shape, bounds = [*shape[:axis], 1, *shape[axis:]], [*bounds[:axis], (0, 1), *bounds[axis:]]
    (Z, Y, X), ((zlo, zhi), (ylo, yhi), (xlo, xhi)) = shape, bounds
    if cfg.BAND:            # full-row bands (hip_band): one band column, x handled inside the kernel
        ntx, nty = 1, max(1, math.ceil(yhi / cfg.BTY))
    else:
        ntx = max(1, math.ceil((X if cfg.XB else xhi) / cfg.TX))
        nty = max(1, math.ceil(yhi / cfg.TY))
    return dict(Z=Z, Y=Y, X=X, zlo=zlo, zhi=zhi, ylo=ylo, yhi=yhi, xlo=xlo, xhi=xhi, ntx=ntx, nty=nty)


def _unaligned_rows(ir, plan, ve, X, dword, all_dword):
    """Rows whose pitch or base is not a multiple of 16 bytes, on 32-bit plane offsets and scalar fields: the config
    of the route that takes them whole — the band's row pieces ('bu'), the LDS-DMA ring's zero-filled ('XM') or
    shifted ('XO') rows — or None (narrower plane-load vectors). ``dword`` / ``all_dword``: the stencil fields and
    halos / all fields start on dwords."""
    esize = 16 // ve
    dword_rows = (X * esize) % 4 == 0 and dword and all_dword
    half_rows = esize == 2 and X % 2 == 1          # fp16 rows on half dwords: realigned in registers ('bo')
    if (dword_rows or half_rows) and _switch('PSAD_BAND_UNALIGNED'):
        # rows whose pitch is not a multiple of 16 bytes on the row-band schedule: row-wise dword-aligned pieces,
        # a 16-byte row pitch in LDS, the partial last chunk stored as dwords (hip_band, 'bu')
        c = plan(ve, True)
        if c.BAND:
            return c
    if not all(np.dtype(f.dtype.numpy_dtype).itemsize == esize for f in ir.fields):
        return None
    xm_rows, xo_rows = (X * esize) % 4 == 0 and dword, esize == 2 and _switch('PSAD_XO')
    probe = plan(ve, False) if xm_rows or xo_rows else None
    ws = ws_geometry(ir, probe) if probe is not None and probe.WS else None
    # rows whose pitch is not a multiple of 16 bytes but of 4 (fp32 / fp64, fp16 with X even): the LDS-DMA
    # ring still takes 16-byte pieces (dword-aligned; the image in LDS keeps its layout) and zero-fills
    # past each row end (XM) — where the WS schedule applies
    xm = xm_rows and probe.ZSUM and ws is not None
    # fp16 rows starting on half dwords (X odd, or an odd-element base): the half-precision LDS-DMA ring
    # loads such rows one element early and shifts them back in LDS (XO) — 255³ fp16 instead of the
    # register-prefetch path
    xo = not xm and xo_rows and ws is not None and ws['kind'] == 'h'
    return replace(probe, XM=True, XO=(1 if X % 2 else 2) if xo else 0) if xm or xo else None


def _route(ir, plan, shape, stencil_align, all_align, restricted):
    """The config of the load path the pointers allow (``_unaligned_rows``, else the widest plane-load vector), or
    None for the one-thread-per-cell schedule."""
    ve0 = 16 // ir.fields[0].dtype.itemsize
    esize, X = 16 // ve0, shape[-1]
    offsets32 = int(np.prod(shape[1:])) * esize < OFFSET_MAX      # (the loader's and the band's 32-bit offsets)

    def fits(v):
        return X % v == 0 and 1 << stencil_align >= v * esize
    if not fits(ve0) and not ir.has_index_dims and offsets32:
        cfg = _unaligned_rows(ir, plan, ve0, X, stencil_align >= 2, all_align >= 2)
        if cfg is not None:
            return cfg
    # widest plane-load vector the rows allow: 16 bytes (and the LDS-DMA loader) when the row pitch is a
    # multiple of 16 bytes, else 8 / 4 bytes (register-prefetch loads) before scalar ones — X = 262
    # fp32: 8-byte loads instead of 4-byte (profiles/r02_misaligned*.log)
    ve = next(v for v in (ve0, ve0 // 2, ve0 // 4, 1) if v >= 1 and fits(v))
    if ve == 1 and ir.ndim == 2 and not restricted and not ir.has_index_dims:
        # 2-D rows of scalar loads: the one-thread-per-cell schedule streams them faster (4097² 5-point
        # 0.028 vs 0.046 ms, 4095×4094 0.027 vs 0.043; profiles/r02_misaligned.log)
        return None
    # the row-band schedule (hip_band): 16-byte pieces and stores on every field and halo, 32-bit plane offsets
    return plan(ve, ve == ve0 and all_align >= 4 and offsets32)


def periodic_march_config(ir, ve, shape=None, tuning=None):
    """The tile of a periodic kernel (3-D, scalar fields): the stencil-class default without the row band, where it
    ends on an LDS-DMA loader (``ws_geometry``: the wrapped plane loads are the loader's,
    ``hip_emitter.loader._ws_piece_offsets``) — else, unless the overrides set ``WS`` themselves, the same tile with the loader on
    (fp32 / fp64 box stencils, whose 'zeros' default is the register-prefetch form), and for fp16 storage last with
    ``CX=4`` as well: the half-precision rings' lanes own quads / pairs of x-adjacent cells, which rows narrower than
    the tile (or a ``CX`` override) would drop; a tile wider than the rows only loads wrapped duplicates — or None."""
    tries = [{}] if 'WS' in _overrides(tuning) else [{}, {'WS': True}]
    if any(storage_ctype(f) == '_Float16' for f in ir.stencil_fields):
        tries.append({'WS': True, 'CX': 4})
    for extra in tries:
        try:
            cfg = default_march_config(ir, ve, shape, {**dict(tuning or {}), **extra}, band=False)
        except ValueError:
            if not extra:
                raise
            continue
        ws = ws_geometry(ir, cfg)
        if ws is not None and ws['lds_bytes'] <= LDS_MAX and not (cfg.BAND or cfg.XM or cfg.XO):
            return cfg
    return None


def _resolve_periodic(ir, tuning, shape, stencil_align):
    """``resolve_march`` for a periodic kernel: ``(config, None)``, or ``(None, why)`` where the launch cannot end on
    an LDS-DMA loader with rows of whole 16-byte pieces (never the band, XM / XO, narrower vectors or the
    register-prefetch fallback: those zero-fill what lies outside the domain)."""
    esize = ir.fields[0].dtype.itemsize
    ve, X = 16 // esize, int(shape[-1])
    if ir.ndim != 3 or ir.has_index_dims:
        return None, 'periodic kernels march only over 3-D scalar fields'
    if (X * esize) % 16:
        return None, f'the row pitch of {X * esize} bytes is not a multiple of 16 bytes'
    if stencil_align < 4:
        return None, f'a stencil field or halo pointer is only {1 << stencil_align}-byte aligned (16 bytes needed)'
    if int(np.prod(shape[1:])) * esize >= OFFSET_MAX:
        return None, "a plane lies beyond the LDS-DMA loader's 32-bit offsets"
    cfg = periodic_march_config(ir, ve, shape, tuning)
    if cfg is None:
        return None, 'no LDS-DMA loader tile applies to this stencil (storage and compute types, LDS size, overrides)'
    return cfg, None


def resolve_march(ir, tuning, shape, stencil_align, all_align, halos=False, z_range=None, z_limits=None,
                  x_border=False, start_signal=False, halo_wait=False):
    """The ``MarchConfig`` of one launch, or None for the one-thread-per-cell schedule. ``stencil_align`` /
    ``all_align``: the lowest ``align_class`` among the stencil fields' tensors and halo planes / among all field
    tensors; ``halos``: halo planes are passed."""
    restricted = halos or z_range is not None or z_limits is not None
    if ir.periodic:
        cfg, why = _resolve_periodic(ir, tuning, shape, stencil_align)
        if cfg is None:
            if restricted or start_signal or halo_wait:
                raise ValueError('halo planes / z ranges / start signals are only supported by the march schedule, '
                                 f'which this launch of a periodic kernel cannot take: {why}')
            return None
        return replace(cfg, SIG=bool(start_signal), HWAIT=bool(halo_wait))
    cfg = _route(ir, lambda ve, band: default_march_config(ir, ve, shape, tuning, band=band), shape, stencil_align,
                 all_align, restricted)
    if cfg is None:
        return None
    if halos and ir.ndim == 2 and cfg.VIEW2D == 'yx':
        cfg = replace(cfg, VIEW2D='zy')
    ws = ws_geometry(ir, cfg)
    # planes beyond the loader's 32-bit buffer offsets: register-prefetch form of the same schedule
    # (never with XM: its rows straddle, which only the loader's zero fill repairs)
    far = ws and int(np.prod(shape[1:])) * max([ncomp(f) for f in ir.stencil_fields] + [1]) * \
        max(ws['esize'], ws.get('ssize', 0)) >= OFFSET_MAX
    if ir.has_index_dims and not cfg.ZSUM and (far or not (cfg.WS and ws)):
        # (vector fields off the zsum schedule: the LDS-DMA plane ring only — the register-prefetch ring takes scalar
        # fields)
        if restricted:
            raise ValueError('vector-field kernels beyond 32-bit plane offsets take no halo planes / z ranges' if far
                             else 'vector-field kernels take halo planes / z ranges only in the zsum schedule')
        return None
    if far:
        assert not cfg.XM
        cfg = ws_fallback_config(cfg)
    xlo, xhi = ir.iteration_bounds(shape)[-1]
    if x_border and cfg.ZSUM and (xlo > 0 or xhi < shape[-1]) and not (ir.ndim == 2 and cfg.VIEW2D == 'zy'):
        cfg = replace(cfg, XB=True)
    if cfg.BAND:
        # unmasked stores when every band row lies in [ylo, yhi) and the x range is whole rows
        g0 = march_extents(ir, shape, cfg, z_range, z_limits)
        whole_x = g0['xlo'] == 0 and g0['xhi'] == g0['X']
        if not (g0['ylo'] == 0 and g0['yhi'] == g0['nty'] * cfg.BTY and whole_x) or g0['X'] % cfg.VE:
            cfg = replace(cfg, BMASK=True, BXW=whole_x and not cfg.XB)       # (X % VE: a partial last chunk per row)
    if halo_wait and not ((cfg.BAND and not (cfg.BREG and shape[-1] % cfg.VE)) or ws_geometry(ir, cfg)):
        raise ValueError('a halo wait needs an LDS-DMA loader (band or WS schedule)')
    return replace(cfg, SIG=bool(start_signal), HWAIT=bool(halo_wait))
