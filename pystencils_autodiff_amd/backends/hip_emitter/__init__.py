"""HIP source emitter for gfx950 (MI355X) stencil kernels.

Replaces the reference's GPU code path — pystencils' CUDA backend printed
through ``framework_integration/printer.py:69-108`` (one thread per cell,
``(16,16,1)`` blocks, every neighbour an L1/L2 load behind a ternary
predicate) — with three schedules written for CDNA4:

``pointwise``
    all accesses at offset 0: flat grid-stride loop, 4 cells per lane, 16-byte
    vector loads/stores (fp32), tail handled per element.

``march`` (2-D and 3-D stencils, the hot path)
    the slowest axis is marched: a workgroup of 4 waves owns a ``TY × TX``
    tile of the two fast axes and walks a chunk of planes along axis 0. Every
    stencil field keeps a ring of ``2·RZ+1`` planes (tile + halo, zero-filled
    outside the domain) in LDS; plane ``z+RZ+1`` is prefetched into registers
    with 16-byte loads while plane ``z`` is computed, so HBM sees each input
    byte about once. Lanes map to consecutive x (wave64 rows), so every tap is
    a conflict-free ``ds_read_b32``; taps shared by the rows a thread owns are
    read once. Out-of-domain planes along axis 0 come from optional halo
    buffers (z-slab exchange, ``parallel``) or are zero. The block index is
    remapped XCD-aware (consecutive tiles on one XCD's L2).

``generic``
    anything else (vector fields, strided tensors, odd dims): one thread per
    cell, runtime strides, per-access bound checks. It is also the schedule the
    parity tests use to cross-check ``march``.

2-D fields run through ``march`` as ``(Y, 1, X)``.
"""
from . import pointwise  # noqa: F401  (the POINTWISE_* switches are read and set as hip_emitter.pointwise.<NAME>)
from .common import PRELUDE, field_params, ncomp, scalar_params, storage_ctype
from .config import MarchConfig
from .generic import emit_generic, emit_zero_border, magic_u32
from .geometry import lite_fields, march_geometry, pair_ok, ws_geometry, zsum_plan
from .loader import extra_params, halo_wait_lines, start_signal_lines, ws_plane_base
from .march import emit_march
from .pointwise import emit_pointwise
from .zsum import emit_zsum

__all__ = ['PRELUDE', 'MarchConfig', 'emit_generic', 'emit_march', 'emit_pointwise', 'emit_zero_border', 'emit_zsum',
           'extra_params', 'field_params', 'halo_wait_lines', 'lite_fields', 'magic_u32', 'march_geometry', 'ncomp',
           'pair_ok', 'scalar_params', 'start_signal_lines', 'storage_ctype', 'ws_geometry', 'ws_plane_base',
           'zsum_plan']
