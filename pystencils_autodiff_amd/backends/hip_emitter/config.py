"""``MarchConfig``: tile shape, pipeline and probe knobs of the marching schedules."""
from dataclasses import dataclass


@dataclass(frozen=True)
class MarchConfig:
    """Tile shape and pipeline of the marching schedule.

    ``CX`` columns of 64 lanes per thread, ``WX`` waves side by side in x
    (``4 // WX`` stacked in y), ``NR`` rows per thread:
    ``TX = 64·CX·WX``, ``TY = (4/WX)·NR``. ``VE`` = elements per vector load
    (16 bytes / element size, or 1 for the unaligned variant). The register-prefetch
    forms load one plane ahead. Knobs no default selects were removed with their
    test rows once measured slower (their logs stay under ``profiles/``).
    """
    CX: int = 2
    WX: int = 1
    NR: int = 2
    VE: int = 4
    NT_STORE: bool = False
    VIEW2D: str = 'yx'          # 2-D fields: 'yx' = (1, Y, X) tiles, 'zy' = march along axis 0 as (Y, 1, X)
    ZSUM: bool = False          # z-partial-sum schedule (``emit_zsum``) instead of the LDS ring
    ZMIN: int = 32              # automatic chunk length: ceil(planes·tiles / BLK) clamped to [ZMIN, ZMAX]
    ZMAX: int = 64
    BLK: int = 512              # target workgroups per launch (≈2 per CU)
    PK: bool = False            # zsum: packed fp32 math (v_pk_fma_f32) over column pairs (CX even, fp32 compute)
    WS: bool = False            # zsum: a fifth (loader) wave streams the planes into an LDS ring by LDS-DMA
                                # (buffer_load … lds), the four compute waves never wait on the VM counter
    D: int = 3                  # WS: planes in flight (ring of D+1 slots), capped by the 6-bit vmcnt
    AR: bool = False            # zsum + PK (columns 64 apart): tap pairs read by ds_read2_b32 offset0:o
                                # offset1:o+64 straight into the packed-FMA register pair (one inline-asm
                                # statement per plane, its own lgkmcnt wait) instead of compiler-merged
                                # adjacent-x reads reshuffled by v_mov
    XB: bool = False            # zsum: also store zeros at x outside [xlo, xhi) in the written rows (tiles
                                # then span all of x) — interior-only kernels behind a zeroed-border output:
                                # whole-line stores instead of partial ones, no separate x-border fill
    NW: int = 4                 # waves per workgroup (not WS): 1 = every wave stages its own tile, the
                                # per-plane workgroup barriers become no-ops
    XM: bool = False            # WS 'dma' ring on rows whose pitch is not a multiple of 16 bytes: the 16-byte pieces
                                # start 4-byte aligned and the last one of a row runs past its end, so the loader
                                # zero-fills the image beyond the row end once a plane has landed
    XO: int = 0                 # with XM, 2-byte elements whose rows start on a half dword: 1 = X odd (every other
                                # row), 2 = X even on an odd-element base (every row of a plane alike). Such a row's
                                # pieces start one element early (LDS-DMA addresses are dword-granular) and the
                                # compute waves realign its dwords in registers (v_alignbit)
    MAP: int = 0                # workgroup → (tile, chunk): 0 = XCD-aware remap, 1 = dispatch order
    BAND: int = 0               # row-band schedule (hip_band.emit_band), fp16: rows per lane; 0 = off
    BTY: int = 8                # band: rows per band (workgroup)
    BX: int = 0                 # band: the row length the kernel is compiled for
    BMASK: bool = False         # band: per-row / per-cell store masks (bounds not whole rows / bands of whole rows)
    BXW: bool = False           # band + BMASK: the launch's x range is the whole row (only y masks and a partial last chunk)
    BTRIM: int = 0              # band: peeled steps without the taps of outputs outside the chunk, 1 = its first two
                                # planes, 2 = its first two and last two
    BEDGE: int = 1              # band probe: 1 = conflict-free edge-dword lanes, 0 = round 3's (2-way per half)
    BNT: int = 2                # band probe: the output stores' cache-policy bits (2 = non-temporal)
    BREG: int = 0               # band, rows of a partial last chunk: padded image filled through registers (no DMA)
    BZF: int = 1                # band, unaligned rows: 1 = the loader zero-fills past each row end, 0 = compute lanes zero
    BPAD: int = 0               # band: 1 = zero-padded image rows, x neighbours read from LDS (no DPP / selects)
    BTAIL: int = 1              # band, rows of a partial last chunk (whole-row stores): the chunk stored as the row's last
                                # VE cells, one shifted 16-byte store (0: a 16-byte store plus dword / half tail stores)
    BFREE: int = 0              # band: 0 = one workgroup barrier per plane; >= 1 = per-plane LDS handshake instead (the
                                # loader publishes each landed plane in an LDS word, each compute wave releases the
                                # planes it has read in its own word), with BFREE - 1 ring slots beyond D + 1.
                                # Measured slower (DESIGN §4 band (19)): opt-in
    SIG: bool = False           # z-slab interior launches: two more parameters (a signal word and a value) after the
                                # extents; workgroup 0 stores the value when the launch starts (start_signal_lines)
    HWAIT: bool = False         # z-slab face launches on the compute stream: a word and a value after the extents (and the
                                # SIG pair); the loader wave waits until the word reaches the value before its first
                                # plane load (halo_wait_lines)
    SLP: int = 0                # march plane ring (nonlinear stencils): 1 = compile with the SLP vectorizer (hipcc's
                                # default), 0 = without (-fno-slp-vectorize: its v_pk_* pairs came with ~300 v_mov per
                                # kernel; hip_kernel.HipStencilKernel.options)
    PD: int = 1                 # march register-prefetch ring: planes in flight in registers (1 or 2: register sets A / B)
    PR: int = 0                 # march plane ring, fp32 arithmetic on scalar fields: lanes own x-adjacent cell pairs
                                # (columns 128 apart) and evaluate the statements on f32x2 (v_pk_fma/mul/add_f32, two
                                # cells per instruction), taps read as ds_read2_b32 pairs, outputs stored as pairs
    SFAST: int = 1              # march ring: a wave whose cells all lie in the written box runs them without per-cell
                                # guards (0: every cell behind its own exec-masked branch). The zsum stores measured
                                # neutral with the same test (profiles/r05_sfast_ab.log) and keep their guards
    BABL: int = 0               # ablation probe (timing only, WRONG RESULTS; set only through march_plan.PROBE_KNOBS,
                                # never a tile key): 1 = one add per row instead of the taps, 2 = no output stores,
                                # 3 = no plane loads (the loader only meets the barriers)

    def __post_init__(self):
        if self.NW not in (1, 2, 4, 8) or self.WX < 1 or self.NW % self.WX:
            raise ValueError(f'NW={self.NW} waves per workgroup must be 1, 2, 4 (or 8 on the LDS-DMA march ring) and '
                             f'a multiple of WX={self.WX}')
        if self.NW == 8 and not (self.WS and not self.ZSUM):
            raise ValueError('NW=8 compute waves only on the LDS-DMA march ring (WS without ZSUM)')

    @property
    def TX(self):
        return 64 * self.CX * self.WX

    @property
    def WY(self):
        return self.NW // self.WX

    @property
    def NT(self):
        """Threads per workgroup of the register-prefetch stencil schedules."""
        return 64 * self.NW

    @property
    def TY(self):
        return self.WY * self.NR
