"""The plan value of the band emitter: everything ``emit_band`` derives before its first printed line."""
from dataclasses import dataclass

from ..printer import KernelExprPrinter
from .geometry import band_esize, band_geometry, band_plans


@dataclass(frozen=True)
class BandTables:
    """What the band printers print from. ``g``: ``band_geometry`` of the row length and band; the row form — at most
    one of ``padded`` (image rows between zero pieces, ``breg``: filled through registers), ``bu`` (rows not a multiple
    of 16 bytes: row-wise pieces, zero fill) and its special case ``bo`` (rows on half dwords); ``W[si]``: the printed
    weight of plan ``si``'s tap (dz, dy, dx); ``cfg``: the knobs the printers read."""
    ir: object
    cfg: object
    g: dict
    S: object                   # the stencil field
    store_field: list           # the field each plan stores
    W: list
    NP: int
    X: int
    TY: int
    R: int
    D: int
    es: int
    half: bool
    et: str                     # storage element type
    vt: str                     # a lane's 16-byte chunk of them
    at: str                     # accumulator slots per (set, row): fp16 = 4 fp32 pairs over the cells (x+a, x+a+4),
    azero: str                  # fp32 = 4 floats
    VE: int
    XP: int                     # row pitch in the LDS image (elements)
    NPR: int                    # pieces per image row
    c0: int                     # image column of a row's first element
    dw: int                     # elements per dword
    NCW: int                    # compute waves
    padded: bool
    breg: bool                  # partial rows on a padded image filled through registers
    partial: bool               # a row's last chunk is partial (stores: tail of X % VE cells)
    bu: bool                    # rows not a multiple of 16 bytes: row-wise pieces, zero fill
    bo: bool                    # rows on half dwords (fp16, X odd): realigned in registers
    czf: bool                   # BZF=0: the first element past a row zeroed in registers
    free: bool                  # LDS handshake instead of the plane barriers
    tail_sb: int                # bytes the row's last chunk lacks
    tail_shift: bool            # the partial last chunk stored as one shifted 16-byte chunk (BTAIL)

    def A(self, si, s, o, a):
        return f'S{si}_{s}_{o}_{a}'

    def operand(self, a, dx):
        return f'P{a + dx + 1}' if self.half else f'H{a + dx + 1}'

    def cell(self, si, s, o, q):
        """Cell q (0..VE-1) of a row's chunk as a storage-type value."""
        if self.half:
            return f'(_Float16){self.A(si, s, o, q % 4)}.{"x" if q < 4 else "y"}'
        return self.A(si, s, o, q)


def band_tables(ir, cfg):
    """The ``BandTables`` of kernel ``ir`` on the band of ``cfg``: eligibility and planning only, no line is printed."""
    if ir.periodic:
        raise ValueError('the band schedule has no periodic form (its row ends and halo planes are zero-filled)')
    plans = band_plans(ir)
    if plans is None:
        raise ValueError('kernel is not eligible for the band schedule')
    fixed = [f for f in ir.fields if f.has_fixed_shape]
    es = band_esize(ir)
    X, TY, R, D = cfg.BX, cfg.BTY, cfg.BAND, cfg.D
    g = band_geometry(X, TY, R, D, es, cfg.BPAD, cfg.BREG, cfg.BFREE)
    padded, breg, VE, XP, CPR = g['padded'], g['reg'], g['VE'], g['XP'], g['CPR']
    assert D * g['NI'] <= 63 and g['NT'] <= 1024, (X, TY, R, D)
    assert not fixed or int(fixed[0].spatial_shape[-1]) == X, 'band kernel compiled for another row length'
    half = es == 2
    partial = X % VE != 0
    bu = not padded and XP != X
    assert not partial or cfg.BMASK, 'rows of a partial last chunk need the masked stores'
    free = bool(cfg.BFREE)
    assert not (free and breg), 'the LDS handshake takes the LDS-DMA loader'
    assert not (cfg.HWAIT and breg), 'the halo wait is the LDS-DMA loader\'s'
    pr = KernelExprPrinter('float', dict(ir.symbol_names))
    W = [{k: f'(float)({pr.doprint_expr(v)})' for k, v in pl['w'].items() if v != 0} for pl in plans]
    at, azero = ('f32x2', '(f32x2)(0.f)') if half else ('float', '0.f')
    # the shifted tail needs a left neighbour chunk of the same row in the same wave for every row group's tail lane
    # (never lane 0 of a wave)
    tail_shift = bool(cfg.BTAIL) and partial and cfg.BXW and CPR >= 2 and \
        all((grp * CPR + CPR - 1) % 64 != 0 for grp in range(g['G']))
    if cfg.BTRIM == 3:
        zc = int(cfg.ZMIN)
        assert cfg.ZMIN == cfg.ZMAX and zc >= 3, 'BTRIM=3 needs a fixed chunk length of >= 3 planes'
    return BandTables(ir=ir, cfg=cfg, g=g, S=ir.stencil_fields[0], store_field=[pl['field'] for pl in plans], W=W,
                      NP=len(plans), X=X, TY=TY, R=R, D=D, es=es, half=half, et='_Float16' if half else 'float',
                      vt='f16x8' if half else 'f32x4', at=at, azero=azero, VE=VE, XP=XP, NPR=XP // VE,
                      c0=VE if padded else 0, dw=4 // es, NCW=g['NCT'] // 64, padded=padded, breg=breg, partial=partial,
                      bu=bu, bo=not breg and (X * es) % 4 != 0, czf=bu and not cfg.BZF, free=free,
                      tail_sb=((VE - X % VE) % VE) * es, tail_shift=tail_shift)
