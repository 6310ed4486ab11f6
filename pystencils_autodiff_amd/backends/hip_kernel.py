"""A compiled GPU stencil kernel: schedule choice, hiprtc build, launch.

Replaces the reference's generated ``call_<kernel>`` wrapper
(``backends/astnodes.py:56-65,143-146``: ``at::Tensor`` → ``data_ptr<T>()``,
then ``kernel<<<grid, block>>>`` from ``indexing.call_parameters``,
``printer.py:88-108``). Calling convention kept: ``kernel(x=..., y=..., z=..., a=5.)``
with every field tensor and scalar passed by name, outputs written in place.
Launches go to torch's current HIP stream (the reference used the legacy
default stream, ``printer.py:106``). Which march kernel a launch gets is decided in ``march_plan`` (host code
without torch or a device, pinned by ``tests/test_march_plan.py``); this module compiles, sizes the grid and packs.
"""
import math
import os

import numpy as np

from . import hip_emitter as he, hip_runtime as rt
from .hip_band import band_geometry, emit_band
from .hip_emitter import (MarchConfig, emit_generic, emit_march, emit_pointwise, emit_zero_border, emit_zsum, magic_u32,
                          march_geometry, ncomp, ws_geometry, zsum_plan)
from .march_plan import (PROBE_KEYS, PROBE_KNOBS, TILE_KEYS, align_class as _align_class,  # noqa: F401 (re-exports)
                         default_march_config, is_pair as _is_pair, march_extents, periodic_march_config, resolve_march,
                         ws_fallback_config)

__all__ = ['HipStencilKernel', 'default_march_config']


def _torch():
    import torch
    return torch


class HipStencilKernel:
    def __init__(self, kernel):
        from .kernel_ir import split_soa
        self.kernel = kernel
        # fzyx vector fields run as one scalar field per component (kernel_ir.split_soa)
        self.ir, self._soa = split_soa(kernel.ir)
        self.name = kernel.function_name
        self._variants = {}            # variant key -> (source, kernel name)
        self._plans = {}               # launch key -> _Plan
        self._specs = None
        self._ref_index = [f.name for f in self.ir.fields].index(self.ir.fields_written[0].name)
        self.last_variant = None
        self.last_plan = None

    # -- sources --------------------------------------------------------------------------------
    def schedule(self):
        ir = self.ir
        if ir.ndim not in (1, 2, 3) or ir.islice is not None:
            return 'generic'               # an iteration_slice: any rectangular subset, bound-checked reads
        if ir.pointwise:
            return 'generic' if ir.has_index_dims else 'pointwise'
        taps = {}
        for r in ir.reads:
            taps.setdefault(r.field, set()).add(r.offsets)
        if ir.stencil_fields and not ir.has_index_dims and all(len(taps.get(f, ())) == 1 for f in ir.stencil_fields):
            # every stencil field read at ONE offset (pull-streaming lattice Boltzmann: component i at -c_i):
            # staging planes in LDS buys no reuse, the one-thread-per-cell schedule streams each component
            return 'generic'
        if ir.periodic:
            # wrapped reads: 3-D scalar-field stencils storing at offset 0 take the march schedules with wrapped
            # LDS-DMA plane loads (where a launch's rows allow, march_plan.resolve_march); everything else — 2-D,
            # vector fields, offset stores — one thread per cell
            if ir.ndim == 3 and ir.stencil_fields and not ir.has_index_dims and \
                    all(all(o == 0 for o in s[1]) for s in ir.stores) and len({f.dtype for f in ir.fields}) == 1:
                return 'march'
            return 'generic'
        if ir.ndim in (2, 3) and all(all(o == 0 for o in s[1]) for s in ir.stores) and \
                len({f.dtype for f in ir.fields}) == 1:
            if ir.has_index_dims:
                # vector fields: the zsum schedule (components interleaved in the plane image) when the
                # stencil is linear off the centre plane, the LDS-DMA plane ring (components interleaved the same
                # way) for other 3-D stencils, else one thread per cell
                probe = MarchConfig(VE=self._vec_elems(), ZSUM=True)
                if ir.stencil_fields and zsum_plan(ir, probe) is not None:
                    return 'march'
                ring = self._march_cfg(self._vec_elems())
                return 'march' if ir.stencil_fields and ring.WS and not ring.ZSUM else 'generic'
            return 'march'
        return 'generic'

    def _vec_elems(self):
        return 16 // self.ir.fields[0].dtype.itemsize

    def _march_cfg(self, ve, shape=None, band=True):
        return default_march_config(self.ir, ve, shape, self.kernel.tuning, band=band)

    def source(self, variant):
        if variant not in self._variants:
            kind = variant[0]
            kname = f"{self.name}_{kind}"
            if kind == 'pointwise':
                src = emit_pointwise(self.ir, kname)
            elif kind == 'march' and variant[1].BAND:
                kname = f"{self.name}_band"
                src = emit_band(self.ir, kname, variant[1])
            elif kind == 'march' and variant[1].ZSUM:
                kname = f"{self.name}_zsum"
                src = emit_zsum(self.ir, kname, variant[1])
            elif kind == 'march':
                src = emit_march(self.ir, kname, variant[1])
            else:
                src = emit_generic(self.ir, kname, idx32='idx32' in variant[1:], contig='contig' in variant[1:],
                                   shared='shared' in variant[1:])
            self._variants[variant] = (src, kname)
        return self._variants[variant]

    def primary_variant(self):
        s = self.schedule()
        if s == 'march':
            shape = None
            fixed = [f for f in self.ir.fields if f.has_fixed_shape]
            if fixed:
                shape = tuple(int(x) for x in fixed[0].spatial_shape)
            if self.ir.periodic:
                cfg = periodic_march_config(self.ir, self._vec_elems(), shape, self.kernel.tuning)
                return ('march', cfg) if cfg is not None else ('generic',)
            return ('march', self._march_cfg(self._vec_elems(), shape))
        return (s,)

    @property
    def code(self):
        return self.source(self.primary_variant())[0]

    @staticmethod
    def options(variant):
        """hiprtc options of a variant: the plane ring of nonlinear stencils (``emit_march``) compiles without the SLP
        vectorizer unless ``SLP=1`` — it paired scalar fp32 ops into ``v_pk_*`` at the price of register moves (varcoef
        fp16 adjoint: 1030 → 871 VALU instructions, 246 → 200 VGPRs); the zsum / band kernels form their packed math
        from explicit vector types and keep the default."""
        if variant[0] == 'march' and not variant[1].ZSUM and not variant[1].BAND and not variant[1].SLP:
            return rt.DEFAULT_OPTIONS + ('-fno-slp-vectorize',)
        return rt.DEFAULT_OPTIONS

    def function(self, variant, device):
        src, kname = self.source(variant)
        code = rt.compile_hip(src, self.options(variant))
        if variant[0] == 'pointwise':
            return {k: rt.load_function(code, f"{kname}_{k}", device) for k in ('v4', 'v1')}
        return rt.load_function(code, kname, device)

    def build(self):
        """Compile the primary variant ahead of time (hiprtc works without a GPU)."""
        v = self.primary_variant()
        return rt.compile_hip(self.source(v)[0], self.options(v))

    # -- launch ---------------------------------------------------------------------------------
    def _field_specs(self):
        if self._specs is None:
            torch = _torch()
            self._specs = [(f.name, getattr(torch, f.dtype.numpy_dtype.name), f.spatial_dimensions + f.index_dimensions,
                            tuple(int(x) for x in f.shape) if f.has_fixed_shape else None) for f in self.ir.fields]
        return self._specs

    def __call__(self, halos=None, stream=None, force_schedule=None, z_range=None, x_border=False, z_limits=None,
                 **kwargs):
        """Launch on the field tensors / scalars given by name.

        ``x_border=True`` asks the zsum schedule to also store zeros at x outside the iteration bounds of
        the rows it writes (returns True if the launch did). ``halos`` = ``{field: (lo_planes, hi_planes)}``: tensors holding the RZ planes just
        below plane 0 / above plane Z-1 of a stencil field (``None`` = zeros, or for a periodic kernel its own far
        planes); ``z_range``
        restricts the written planes of axis 0 — ``(lo, hi)``, or two disjoint ranges of equal
        length ``((lo0, hi0), (lo1, hi1))`` written by ONE launch (the two slab faces; both:
        z-slab decomposition, ``zslab.py``). ``z_limits=(lo, hi)`` replaces the kernel's own axis-0
        iteration bounds (an interior-only kernel on a z-slab: the GLOBAL domain's interior, in local
        plane numbers).
        The first call for a given (shape, alignment, halo layout, z range) builds a launch plan
        (variant, function handle, grid, argument layout); later calls only re-pack pointers.
        """
        prep = self.prepare(halos=halos, force_schedule=force_schedule, z_range=z_range, x_border=x_border,
                            z_limits=z_limits, **kwargs)
        if prep is None:
            return None
        fn, grid, block, packed, xb, device = prep
        if grid == 0:
            return xb
        torch = _torch()
        if stream is None:
            stream = torch._C._cuda_getCurrentRawStream(device)
        if device != torch.cuda.current_device():
            # the function handle belongs to the module loaded on the tensors' device: launch with it current
            with torch.cuda.device(device):
                rt.launch(fn, (grid,), (block,), packed, stream)
        else:
            rt.launch(fn, (grid,), (block,), packed, stream)
        return xb

    def prepare(self, halos=None, force_schedule=None, z_range=None, x_border=False, z_limits=None,
                start_signal=False, halo_wait=False, **kwargs):
        """Everything of a launch but the launch: ``(function, grid, block, packed args, x_border done,
        device)``, or None for an empty domain (arguments as for ``__call__``). ``start_signal=True`` (march
        schedules, the z-slab interior): the kernel takes a signal word and a value after its extents, both zero in
        the packed arguments (no store) — the caller patches them at ``last_plan.sig_offsets``. ``halo_wait=True``
        (LDS-DMA loader schedules, the z-slab faces on the compute stream): the loader waits for a word to reach a
        value before its first plane load; both zero (no wait) until patched at ``last_plan.hwait_offsets``; a plan
        without an LDS-DMA loader raises ``ValueError``."""
        torch = _torch()
        ir = self.ir
        if self._soa:
            kwargs = self._bind_components(kwargs)
        tensors = []
        for name, dtype, ndim, fixed in self._field_specs():
            t = kwargs.get(name)
            if t is None:
                raise TypeError(f"{self.name}: missing field argument '{name}'")
            if not isinstance(t, (torch.Tensor, _Plane)) or not t.is_cuda:
                raise TypeError(f"{self.name}: field '{name}' must be a torch tensor on the GPU")
            if t.dtype != dtype:
                raise TypeError(f"{self.name}: field '{name}' has dtype {t.dtype}, kernel expects {dtype}")
            if t.dim() != ndim:
                raise ValueError(f"{self.name}: field '{name}' expects {ndim} dims, got {t.dim()}")
            if fixed is not None and tuple(t.shape) != fixed:
                raise ValueError(f"{self.name}: field '{name}' was declared with shape {fixed}, got {tuple(t.shape)}")
            tensors.append(t)
        scalars = []
        for s_ in ir.scalars:
            if s_.name not in kwargs:
                raise TypeError(f"{self.name}: missing scalar argument '{s_.name}'")
            scalars.append(float(kwargs[s_.name]))
        ref = tensors[self._ref_index]
        shape = tuple(ref.shape[:ir.ndim])
        for t, (name, _, _, _) in zip(tensors, self._specs):
            if tuple(t.shape[:ir.ndim]) != shape:
                raise ValueError(f"{self.name}: field '{name}' has spatial shape {tuple(t.shape[:ir.ndim])}, "
                                 f"expected {shape}")
        if any(n == 0 for n in shape):
            return None
        device = ref.device.index
        halo_list = []
        if halos:
            for f in ir.stencil_fields:
                lo, hi = halos.get(f.name, (None, None))
                halo_list += [lo, hi]
        ptrs = [t.data_ptr() for t in tensors]
        hptrs = [h.data_ptr() if h is not None else 0 for h in halo_list]
        contiguous = all(t.is_contiguous() for t in tensors)
        strides = None if contiguous else tuple(tuple(t.stride()) for t in tensors)
        # the alignment CLASS of every pointer (trailing zero bits, capped at 32 bytes): the plan's load path
        # depends on 16-, 8-, 4- and 2-byte alignment (LDS-DMA ring, narrower vectors, XM rows), so a plan built
        # for one class must not serve a pointer of another
        align = tuple(_align_class(p) for p in ptrs + hptrs)
        key = (force_schedule, bool(x_border), shape, strides, align,
               tuple(h.numel() if h is not None else -1 for h in halo_list), _zkey(z_range),
               tuple(z_limits) if z_limits is not None else None, device) + (('sig',) if start_signal else ()) + \
            (('hwait',) if halo_wait else ())
        plan = self._plans.get(key)
        if plan is None:
            if z_limits is not None:
                if not ir.ndim == 3 or not 0 <= int(z_limits[0]) <= int(z_limits[1]) <= shape[0]:
                    raise ValueError(f'z_limits {z_limits} must lie in [0, {shape[0]}] of a 3-D kernel')
            plan = self._make_plan(tensors, halo_list, shape, device, contiguous, force_schedule, z_range, x_border,
                                   z_limits, start_signal, halo_wait)
            self._plans[key] = plan
        self.last_variant = plan.variant
        self.last_plan = plan
        if plan.grid == 0:
            return plan.fn, 0, plan.block, b'', plan.xb, device
        return plan.fn, plan.grid, plan.block, plan.pack(ptrs, hptrs, scalars), plan.xb, device

    def _bind_components(self, kwargs):
        """fzyx vector tensors → one plane per component (``split_soa``'s scalar fields); any strides are
        accepted (a component whose plane is not C-contiguous takes the generic schedule). The planes are
        ``_Plane`` records (pointer arithmetic on the parent), not torch views: a D3Q19 adjoint binds 57
        planes per launch, ~4 µs of host time each as views."""
        torch = _torch()
        kwargs = dict(kwargs)
        sdim = self.ir.ndim
        for name, comps in self._soa.items():
            t = kwargs.pop(name, None)
            if t is None:
                raise TypeError(f"{self.name}: missing field argument '{name}'")
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{self.name}: field '{name}' must be a torch tensor on the GPU")
            nidx = len(comps[0][1])
            if t.dim() != sdim + nidx:
                raise ValueError(f"{self.name}: field '{name}' expects {sdim + nidx} dims, got {t.dim()}")
            shape, strides = tuple(t.shape), tuple(t.stride())
            base, esize = t.data_ptr(), t.element_size()
            for cfield, idx in comps:
                if any(not 0 <= i < n for i, n in zip(idx, shape[sdim:])):
                    raise ValueError(f"{self.name}: field '{name}' has component shape {shape[sdim:]}")
                off = sum(i * st for i, st in zip(idx, strides[sdim:]))
                kwargs[cfield.name] = _Plane(t, base + off * esize, shape[:sdim], strides[:sdim])
        return kwargs

    def _make_plan(self, tensors, halo_list, shape, device, contiguous, force_schedule, z_range, x_border=False,
                   z_limits=None, start_signal=False, halo_wait=False):
        torch = _torch()
        ir = self.ir
        sched = force_schedule or self.schedule()
        if sched != 'generic' and not contiguous:
            sched = 'generic'
        if (halo_list or z_range is not None or z_limits is not None or start_signal or halo_wait) and \
                sched != 'march':
            raise ValueError('halo planes / z ranges / start signals are only supported by the march schedule')
        with torch.cuda.device(device):
            if sched == 'pointwise':
                return self._plan_pointwise(tensors, shape, device)
            if sched == 'march':
                return self._plan_march(tensors, halo_list, shape, device, z_range, x_border, z_limits, start_signal,
                                        halo_wait)
            return self._plan_generic(tensors, shape, device)

    def _scalar_kind(self):
        return 'f64' if self.ir.compute_dtype == np.float64 else 'f32'

    def _plan_pointwise(self, tensors, shape, device):
        fns = self.function(('pointwise',), device)
        n = int(np.prod(shape))
        aligned = all(t.data_ptr() % 32 == 0 for t in tensors)
        per_block = 256 * (4 * he.pointwise.POINTWISE_UNROLL if aligned else 1)
        cap = (he.pointwise.POINTWISE_MAX_BLOCKS or 2 ** 31 - 1) if aligned else 256 * 16
        blocks = max(1, min(math.ceil(n / per_block), cap))
        kinds = ['ptr'] * len(tensors) + ['i64'] + [self._scalar_kind()] * len(self.ir.scalars)
        return _Plan(('pointwise', 'v4' if aligned else 'v1'), fns['v4' if aligned else 'v1'], blocks, kinds,
                     len(tensors), 0, [n])

    def _plan_generic(self, tensors, shape, device):
        ir = self.ir
        if ir.periodic and any(r >= int(n) for r, n in zip(ir.radius, shape)):
            raise ValueError(f'periodic kernel: stencil radius {ir.radius} must be below the extent {shape}')
        bounds = ir.iteration_bounds(shape)
        ncell = int(np.prod([hi - lo for lo, hi in bounds]))
        idx32 = 0 < ncell < 2 ** 31
        contig = all(t.is_contiguous() for t in tensors)
        # one shape and one set of strides for every tensor, offsets within 32 bits: shared 32-bit addressing
        reach = max(list(ir.radius) + [0]) + 1
        shared = len({(tuple(t.shape), tuple(t.stride())) for t in tensors}) == 1 and \
            sum(abs(int(st)) * (int(n) - 1 + reach) for st, n in zip(tensors[0].stride(), tensors[0].shape)) < 2 ** 31 - 1
        variant = ('generic',) + (('idx32',) if idx32 else ()) + (('contig',) if contig else ()) + \
            (('shared',) if shared else ())
        fn = self.function(variant, device)
        statics = [int(n) for n in shape]
        for t in (tensors[:1] if shared else tensors):
            statics += [int(s_) for s_ in t.stride()]
        kinds = ['ptr'] * len(tensors) + ['i64'] * len(shape) + ['i32' if shared else 'i64'] * (len(statics) - len(shape))
        for lo, hi in bounds:
            statics += [lo, hi]
            kinds += ['i64', 'i64']
        if idx32:
            extra = [ncell]
            kinds.append('u32')
            for lo, hi in bounds[1:]:
                m, sh = magic_u32(max(1, hi - lo))
                extra += [m, sh]
                kinds += ['u32', 'i32']
            statics += extra
        kinds += [self._scalar_kind()] * len(ir.scalars)
        blocks = max(1, min(math.ceil(ncell / 256), 256 * 64)) if ncell > 0 else 0
        return _Plan(variant, fn, blocks, kinds, len(tensors), 0, statics)

    def _resident_slots(self, fn, block, device):
        """Workgroups of this kernel resident on the whole GPU at once (LDS, VGPR and wave limits per CU
        × CU count), from the loaded code object's attributes."""
        torch = _torch()
        a = rt.function_attributes(fn)
        regs, lds = a['num_regs'], a['shared_bytes']
        waves = -(-block // 64)
        per_simd = max(1, min(8, 512 // max(8, -(-regs // 8) * 8)))
        per_cu = max(1, min(4 * per_simd // waves, 163840 // max(1, lds), 32 // waves))
        return per_cu * torch.cuda.get_device_properties(device).multi_processor_count

    @staticmethod
    def quantized_chunk(nz, nt, slots, zmin, zmax, rz, wsat):
        """Chunk length for the WS schedule (few resident workgroups, each with a fixed number of bytes
        in flight): the chunk count c minimising Σ_rounds (planes per chunk + halo + fill) ·
        max(1, active / wsat) — a round takes at least one workgroup's march (latency bound below
        ``wsat`` concurrent workgroups, bandwidth bound above). The short last round of 128-plane
        chunks is what makes 768³ slower per cell than 1024³ (profiles/r01_tune_odd_sizes.log)."""
        best = None
        c0 = max(1, -(-nz // zmax))
        for c in range(c0, max(c0, nz // max(1, zmin)) + 1):
            zc = -(-nz // c)
            n = nt * -(-nz // zc)
            full, rem = divmod(n, slots)
            t = (zc + 2 * rz + 2) * (full * max(1.0, slots / wsat) + (max(1.0, rem / wsat) if rem else 0.0))
            if best is None or t < best[0] - 1e-9:
                best = (t, zc)
        return best[1]

    def march_launch_geometry(self, shape, cfg, z_range=None, slots=None, z_limits=None):
        """(Z, Y, X), bounds and grid of the march schedule for a field shape; ``slots`` = resident
        workgroups (``_resident_slots``) switches the WS schedule to quantisation-aware chunks."""
        ir = self.ir
        geo = march_extents(ir, shape, cfg, z_range, z_limits)
        nt, nz = geo['ntx'] * geo['nty'], max(0, geo['zhi'] - geo['zlo'])
        if z_range is not None and _is_pair(z_range):       # the two faces: one chunk each, zstep planes apart
            (a0, a1), (b0, _) = z_range
            return dict(geo, zc=int(a1) - int(a0), zstep=int(b0) - int(a0), grid=2 * nt)
        # chunk length: aim at ~2 workgroups per CU (512 blocks), ZMIN..ZMAX planes per chunk (each chunk
        # re-reads 2·RZ halo planes). 7-point 1024³, 128×32 tiles: 64-plane chunks 1.536 ms vs 128-plane
        # 1.570 ms (profiles/r01_tune_cx_ab_1024.log); 512³ and 128×1024² slabs land on 64 by the target
        env_zc, env_blocks = os.environ.get('PSAD_MARCH_ZC'), os.environ.get('PSAD_MARCH_BLOCKS')
        target = int(self.kernel.tuning.get('BLOCKS', cfg.BLK if env_blocks is None else env_blocks))
        zc = self.kernel.tuning.get('ZC') or int(0 if env_zc is None else env_zc) or \
            min(nz, max(cfg.ZMIN, min(cfg.ZMAX, math.ceil(nz * nt / target))))
        explicit = self.kernel.tuning.get('ZC') or env_zc or 'BLOCKS' in self.kernel.tuning or env_blocks
        cus = _torch().cuda.get_device_properties(_torch().cuda.current_device()).multi_processor_count \
            if slots else 0
        # measured on the default WS tiles (one workgroup per CU, or the half-width tiles it picks for
        # x extents that pad less); with user tile / depth overrides that allow several partially filled
        # workgroups per CU it can pick an unbalanced grid (512³ D=3: 0.249 vs 0.188 ms), so those keep
        # the block-count target
        overridden = any(k in self.kernel.tuning for k in ('CX', 'NR', 'D', 'WX', 'NW'))
        # (not for the 2-D row ring, whose block-count target measured faster: 2-D varcoef 4096² fp32 adjoint 0.072 vs
        # 0.085 ms, profiles/r06_nl2d_zy.log)
        rows2d = ir.ndim == 2 and not cfg.ZSUM
        if slots and cfg.WS and nz and not explicit and (slots <= cus or not overridden) and not rows2d:
            ws = ws_geometry(ir, cfg)
            # workgroups that saturate HBM: ~64 KiB in flight per CU (one 256×16 fp32 ring of 4 planes)
            wsat = max(cus, math.ceil(cus * 65536 / (ws['D'] * ws['per_plane'] * 1024)))
            zc = self.quantized_chunk(nz, nt, slots, cfg.ZMIN, cfg.ZMAX, march_geometry(ir, cfg)['RZ'], wsat)
        zc = min(zc, nz) if nz else zc
        zc = max(zc, min(nz, 4 * max(1, march_geometry(ir, cfg)['RZ'])))
        nchunks = math.ceil(nz / zc) if nz else 0
        if nchunks:
            # equal chunks: same chunk count (same halo re-reads), no short tail chunk — 27-point fp16
            # 192×768² slab: 27 → 24 planes, 0.129 → 0.113 ms (profiles/r01_tune_zc_slab.log)
            zc = math.ceil(nz / nchunks)
        return dict(geo, zc=zc, zstep=zc, grid=nt * nchunks)

    def _plan_march(self, tensors, halo_list, shape, device, z_range, x_border=False, z_limits=None,
                    start_signal=False, halo_wait=False):
        ir = self.ir
        if ir.periodic and any(r >= int(n) for r, n in zip(ir.radius, shape)):
            raise ValueError(f'periodic kernel: stencil radius {ir.radius} must be below the extent {shape}')
        stencil = ir.stencil_fields
        by_name = {f.name: t for f, t in zip(ir.fields, tensors)}
        read = [by_name[f.name] for f in stencil] + [h for h in halo_list if h is not None]
        cfg = resolve_march(ir, self.kernel.tuning, shape, min([_align_class(t.data_ptr()) for t in read] + [5]),
                            min(_align_class(t.data_ptr()) for t in tensors), bool(halo_list), z_range, z_limits,
                            x_border, start_signal, halo_wait)
        if cfg is None:
            return self._plan_generic(tensors, shape, device)
        variant = ('march', cfg)
        fn = self.function(variant, device)
        ws = ws_geometry(ir, cfg)
        slots = self._resident_slots(fn, ws['block'], device) if ws else None
        geo = self.march_launch_geometry(shape, cfg, z_range, slots=slots, z_limits=z_limits)
        grid = geo['grid'] if geo['yhi'] > geo['ylo'] and geo['xhi'] > geo['xlo'] else 0
        rz = march_geometry(ir, cfg)['RZ']
        for i, f in enumerate(stencil):
            for h in (halo_list[2 * i:2 * i + 2] if halo_list else ()):
                if h is not None and (not isinstance(h, _torch().Tensor) or not h.is_contiguous() or
                                      h.numel() < rz * geo['Y'] * geo['X'] * ncomp(f) or
                                      h.dtype != by_name[f.name].dtype or h.device != by_name[f.name].device):
                    raise ValueError(f"halo for '{f.name}' must be a contiguous tensor of >= {rz} planes "
                                     "on the field's device")
        if max(geo['Z'], geo['Y'], geo['X']) >= 2 ** 31 or grid >= 2 ** 31:
            raise ValueError('field extent too large for the march schedule')
        statics = [int(geo[k]) for k in 'Z Y X zlo zhi ylo yhi xlo xhi zc zstep ntx nty'.split()]
        kinds = ['ptr'] * (len(tensors) + 2 * len(stencil)) + ['i32'] * len(statics)
        for _ in range(cfg.SIG + cfg.HWAIT):    # the start signal, the halo wait: word and value, patched by the caller
            kinds += ['ptr', 'u32']
            statics += [0, 0]
        kinds += [self._scalar_kind()] * len(ir.scalars)
        block = ws['block'] if ws else cfg.NT if not cfg.BAND else \
            band_geometry(cfg.BX, cfg.BTY, cfg.BAND, cfg.D, 16 // cfg.VE, cfg.BPAD, cfg.BREG, cfg.BFREE)['NT']
        plan = _Plan(variant, fn, grid, kinds, len(tensors), 2 * len(stencil), statics, xb=cfg.XB, block=block)
        i = len(tensors) + 2 * len(stencil) + 13
        if cfg.SIG:
            plan.sig_offsets = (plan.offsets[i], plan.offsets[i + 1])
            i += 2
        if cfg.HWAIT:
            plan.hwait_offsets = (plan.offsets[i], plan.offsets[i + 1])
        return plan


class _Plane:
    """One component plane of an fzyx tensor, as the launch path sees a tensor: pointer, shape, strides,
    dtype, device (and the parent, kept alive for the duration of the call)."""
    __slots__ = ('parent', 'ptr', 'shape', 'strides', 'dtype', 'device', 'is_cuda')

    def __init__(self, parent, ptr, shape, strides):
        self.parent = parent
        self.ptr = ptr
        self.shape = shape
        self.strides = strides
        self.dtype = parent.dtype
        self.device = parent.device
        self.is_cuda = parent.is_cuda

    def data_ptr(self):
        return self.ptr

    def dim(self):
        return len(self.shape)

    def stride(self):
        return self.strides

    def numel(self):
        n = 1
        for v in self.shape:
            n *= v
        return n

    def element_size(self):
        return self.parent.element_size()

    def is_contiguous(self):
        expect = 1
        for n, st in zip(reversed(self.shape), reversed(self.strides)):
            if n != 1 and st != expect:
                return False
            expect *= n
        return True


def _zkey(z_range):
    if z_range is None:
        return None
    return tuple(tuple(int(v) for v in r) for r in z_range) if _is_pair(z_range) else tuple(int(v) for v in z_range)


class _Plan:
    """A resolved launch: variant, function handle, grid and a struct that packs the argument
    buffer (pointers, then static extents, then scalars) at HIP_LAUNCH_PARAM_BUFFER alignment."""

    _CODES = {'ptr': ('Q', 8), 'i32': ('i', 4), 'u32': ('I', 4), 'i64': ('q', 8), 'f32': ('f', 4), 'f64': ('d', 8)}

    def __init__(self, variant, fn, grid, kinds, n_ptr, n_halo, statics, block=256, xb=False):
        import struct
        self.variant = variant
        self.fn = fn
        self.grid = grid
        self.block = block
        self.xb = xb                     # the launch also zeroes x outside the iteration bounds
        fmt, off = '<', 0
        self.kinds, self.offsets = list(kinds), []       # byte offset of every argument in the packed buffer
        for k in kinds:
            c, size = self._CODES[k]
            pad = (-off) % size
            fmt += 'x' * pad + c
            self.offsets.append(off + pad)
            off += pad + size
        fmt += 'x' * ((-off) % 8)
        self.struct = struct.Struct(fmt)
        self.n_ptr = n_ptr
        self.n_halo = n_halo
        self.statics = list(statics)
        self.sig_offsets = None          # (byte offset of the start-signal word, of its value): SIG launches
        self.hwait_offsets = None        # (byte offset of the halo-wait word, of its value): HWAIT launches

    def scalar_slots(self, n):
        """``(byte offset, is f64)`` of the last ``n`` arguments (the kernel's scalar parameters)."""
        return [(o, k == 'f64') for o, k in zip(self.offsets[len(self.offsets) - n:], self.kinds[len(self.kinds) - n:])] \
            if n else []

    def pack(self, ptrs, hptrs, scalars):
        return self.struct.pack(*ptrs, *(hptrs if hptrs else [0] * self.n_halo), *self.statics, *scalars)


_zero_border_fns = {}


def zero_border(t, bounds, ncomp=1, stream=None, x=True, zy=True):
    """Zero, in one launch on the current stream, every cell of the contiguous GPU tensor ``t`` outside the
    per-axis ``[lo, hi)`` ``bounds`` of its spatial axes (components, if any, last) — the border an
    interior-only kernel leaves to the reference's ``torch.zeros`` allocation. ``x=False`` leaves the x
    ends of the rows (written by an ``x_border`` launch), ``zy=False`` does only those."""
    import struct
    torch = _torch()
    nd = len(bounds)
    shape = [int(s) for s in t.shape[:nd]]
    bounds = [(int(a), int(b)) for a, b in bounds]
    if not x:
        bounds[-1] = (0, shape[-1])
    if not zy:
        bounds[:-1] = [(0, n) for n in shape[:-1]]
    while len(shape) < 3:
        shape.insert(0, 1)
        bounds.insert(0, (0, 1))
    (zlo, zhi), (ylo, yhi), (xlo, xhi) = bounds
    Z, Y, X = shape
    L = X * ncomp
    total = (Z - (zhi - zlo)) * Y * L + (zhi - zlo) * (Y - (yhi - ylo)) * L + \
        (zhi - zlo) * (yhi - ylo) * (L - (xhi - xlo) * ncomp)
    if total <= 0:
        return
    if not t.is_contiguous() or t.numel() != Z * Y * L:
        raise ValueError('zero_border needs a contiguous tensor of the kernel shape')
    device = t.device.index
    idx32 = Z * Y * L + 256 * 256 * 64 < 2 ** 31
    key = (t.element_size(), idx32, device)
    fn = _zero_border_fns.get(key)
    if fn is None:
        src, name = emit_zero_border(t.element_size(), idx32)
        fn = _zero_border_fns[key] = rt.load_function(rt.compile_hip(src), name, device)
    if stream is None:
        stream = torch._C._cuda_getCurrentRawStream(device)
    args = struct.pack('<Q9q', t.data_ptr(), Z, Y, L, zlo, zhi, ylo, yhi, xlo * ncomp, xhi * ncomp)
    rt.launch(fn, (min(math.ceil(total / 256), 256 * 64),), (256,), args, stream)
