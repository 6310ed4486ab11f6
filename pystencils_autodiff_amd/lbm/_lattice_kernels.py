"""The lattice Boltzmann schedule: stream-pull-collide SRT forward and adjoint kernels, written for the lattice.

``AutoDiffLatticeBoltzmannStep`` drives rules made by ``create_lb_update_rule`` (lbmpy's SRT
``stream_pull_collide`` kernel [ext], ``/root/reference/src/pystencils_autodiff/lbm/_autodiff_lbstep.py:189-247,
372-398``) through these kernels instead of the general one-thread-per-cell lowering of the rule's
``AssignmentCollection``: the general lowering reads and writes each pdf component as its own field, in the
layout of the caller's tensors, with every cell's 2·Q streams in Q separate component planes.

What this schedule does differently:

* **Layouts by strides.** A pdf array is addressed as ``q·s_q + z·s_z + y·s_y + x·s_x``: the caller's fzyx
  (lbmpy's default, one plane per component) or AoS arrays are read and written in place. The time-step op's
  intermediate states, which only the op sees, use the row-interleaved layout ``[z][y][q][x]``: the Q
  components of a lattice row are one contiguous block (Q·X elements), so a wave's 2·Q accesses per row land
  in ~10 neighbouring row blocks instead of 2·Q planes a whole field apart.
* **Walls.** An optional flag array (``uint8``, one per cell, C order, 1 = no-slip obstacle) turns on lbmpy's
  half-way bounce-back fused into the pull: ``f_i(x) = src_ī(x)`` where ``x − c_i`` is an obstacle
  (``lbmpy.boundaries.NoSlip`` [ext] writes ``src_ī(x + c_i) := src_i(x)`` into the obstacle cell before the
  pull, ``adjoint_boundaryconditions.py:49-72`` moves the adjoint back); obstacle cells keep their state
  (``dst = src`` there — lbmpy's values in obstacle cells are not part of the flow).
* **Adjoint in scatter form through the collision's structure** (``_method.create_lb_adjoint_rule``):
  ``v_j = (1 − ω) g_j + ω (A + Σ_a B_a ∂u_a/∂f_j)`` with two moment-like sums, stored to the cell the forward
  pulled ``f_j`` from — ``(x − c_j, j)``, or ``(x, ī)`` for a bounced ``f_j``. Every (component, cell) of
  the result is written exactly once (for fluid ``x``: by ``x + c_k`` if that cell is fluid, else by ``x``
  itself; obstacle cells by themselves), so the output needs no zero fill and no atomics.

One source is printed for both targets (``_lattice_source``): a HIP kernel (one thread per cell, wave64 along x)
compiled by hiprtc, and a C loop nest (``use_cuda=False`` / ``target='cpu'``) compiled by gcc. This module holds the
host side: masks and cell lists, compiling, argument buffers and launches.
"""
import ctypes
import dataclasses
import os
import struct

import numpy as np

from ._lattice_source import FIX_BIT, FIX_BLOCK, SELF_BIT, LatticeSource, emit  # noqa: F401 (the bits: re-exported)

__all__ = ['LatticeKernels', 'LaunchPlan', 'lattice_strides', 'row_interleaved_empty', 'neighbour_mask']


def fix_cells(flags, stencil, program_ids, programs=None):
    """Bool over the domain: fluid cells with a neighbour ``x − c_i`` (periodic) among the walls of ``program_ids``
    (the flag ids whose boundary is a link program) — the cells the HIP fix-up kernels recompute. ``programs`` (per
    flag id None or its link program): also every fluid cell ``x + c_o`` that a neighbour link of such a cell ``x``
    reads, and so adds its adjoint into (whether or not the link is taken there: a superset costs a thread)."""
    f = np.asarray(flags)
    axes = tuple(range(f.ndim))
    prog = np.isin(f, np.asarray(sorted(program_ids), dtype=f.dtype))
    near = np.zeros(f.shape, bool)
    for c in stencil.directions:
        if any(c):
            near |= np.roll(prog, tuple(int(v) for v in c), axis=axes)
    fluid = f == 0
    for wid, pg in enumerate(programs or ()):
        for d, row in enumerate(pg or ()):
            if row is None or len(row) < 4 or not row[3]:
                continue
            # the fluid cells x whose link of direction d ends in a wall cell of this id: x + c_d
            src = fluid & np.roll(f == wid, tuple(-int(v) for v in stencil.directions[d]), axis=axes)
            for o in row[3]:
                near |= np.roll(src, tuple(int(v) for v in stencil.directions[o]), axis=axes)
    return near & fluid


def neighbour_mask(flags, stencil, xp, fix=None):
    """``uint32`` per cell: bit i set where ``x − c_i`` is a wall cell (periodic), bit ``SELF_BIT`` where ``x`` is
    one (``flags``: wall ids over the domain, 0 = fluid, numpy or torch); bit ``FIX_BIT`` where ``fix`` (a numpy
    bool array, ``fix_cells``) is set — then computed on the host, and a torch result comes back as the uint32
    bits in an int32 tensor on ``flags``' device."""
    is_torch = xp.__name__ == 'torch'
    if fix is not None:
        m = neighbour_mask(flags.cpu().numpy() if is_torch else flags, stencil, np)
        m = m | (np.asarray(fix, bool).astype(np.uint32) << np.uint32(FIX_BIT))
        return xp.from_numpy(np.ascontiguousarray(m).view(np.int32)).to(flags.device) if is_torch else m
    f = (flags != 0).to(xp.int32) if is_torch else (np.asarray(flags) != 0).astype(np.int64)
    m = f * 0
    for i, c in enumerate(stencil.directions):
        if not any(c):
            continue
        r = f
        for ax, sh in enumerate(c):
            if sh:
                r = xp.roll(r, shifts=sh, dims=ax) if is_torch else np.roll(r, sh, axis=ax)
        m = m | (r << i)
    m = m | (f << SELF_BIT)
    return m.to(xp.int32).contiguous() if is_torch else np.ascontiguousarray(m.astype(np.uint32))


def lattice_strides(t, D):
    """``(s_q, s_z, s_y, s_x)`` in elements of a pdf tensor ``[*spatial, q]`` (2-D: ``s_z`` = 0)."""
    st = [int(s) for s in (t.stride() if hasattr(t, 'stride') and callable(t.stride) else
                           [s // t.itemsize for s in t.strides])]
    sp_ = st[:D]
    if D == 2:
        sp_ = [0] + sp_
    return (st[D],) + tuple(sp_)


def row_interleaved_empty(domain, Q, dtype, device):
    """An uninitialised pdf tensor ``[*domain, Q]`` in the row-interleaved layout ``[z][y][q][x]`` (each lattice
    row's Q components one contiguous block) — the time-step op's internal states."""
    import torch
    dims = list(domain)
    base = torch.empty(dims[:-1] + [Q, dims[-1]], dtype=dtype, device=device)
    return base.transpose(-1, -2)


class LatticeKernels:
    """Compiled forward / adjoint lattice kernels of one (stencil, compressible, dtype, walls, links, target).
    ``mask`` arguments are the cells' neighbour masks (``neighbour_mask``), ``None`` without walls; ``ids`` the
    cells' wall ids (the ``uint8`` flag array, C order) when ``links`` is given (walls other than plain
    bounce-back)."""

    def __init__(self, stencil, compressible, dtype, walls, target, links=None, force_model=None, force=None,
                 force_field=False, trt=None, programs=None, mrt=None, *, omega_field=False, zero_centered=False,
                 smagorinsky=None):
        self.stencil = stencil
        # the Smagorinsky constant C_s (None: no subgrid model): a constant of the emitted source, so of every cache
        # key made from it
        self.smagorinsky = None if smagorinsky is None else float(smagorinsky)
        # the state arrays hold f_i − w_i (``LatticeSource.zero_centered``); the adjoint arrays are not shifted
        self.zero_centered = bool(zero_centered)
        # ω read per cell from a scalar field ``[*domain]``, its adjoint accumulated by the adjoint launches
        self.omega_field = bool(omega_field)
        # MRT: (P_ω, C) relaxation matrices as float tuples (``_method.mrt_relaxation_matrices``)
        self.mrt = None if mrt is None else tuple(tuple(tuple(float(v) for v in row) for row in M) for M in mrt)
        self.trt = None if trt is None else (str(trt[0]), float(trt[1]))
        self.force_model = force_model
        self.force_field = bool(force_model) and bool(force_field)
        self.force = None if force_model is None or self.force_field else tuple(float(v) for v in force)
        self.compressible = bool(compressible)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.float16, np.float32, np.float64):
            raise NotImplementedError(f'lattice kernels for {self.dtype} pdfs')
        # the compute type (float16 storage computes in float32; ω is passed in it)
        self.ct = 'double' if self.dtype == np.float64 else 'float'
        self.walls = bool(walls)
        self.links = links if walls else None
        self.target = target
        # what to print (``source`` fills in the index type, the addressing and the adjoint mode)
        self.spec = spec = LatticeSource(
            stencil, self.compressible, self.ct, self.walls, self.links, programs, force_model, self.force,
            self.force_field, self.trt, self.mrt, target='hip' if target == 'gpu' else 'c',
            omega_field=self.omega_field, zero_centered=self.zero_centered, half=self.dtype == np.float16,
            smagorinsky=self.smagorinsky)
        # density-weighted links: the adjoint takes a second pass (lbm_adj_rho) over a per-cell scratch array
        self.rho_links = spec.rho_links
        # link programs (boundaries.link_program). C: inline, a Q-component scratch array per cell and the second
        # pass; HIP: the main kernels skip the FIX_BIT cells, the fix-up kernels (a module of their own) redo them
        self.programs = programs if spec.gen else None
        self.link_pass = self.rho_links or (self.programs is not None and target != 'gpu')
        self.program_ids = tuple(k for k, p in enumerate(self.programs or ()) if p is not None)
        self._rho_bufs = {}
        self._fns = {}
        self._plans = {}

    def source(self, idx='int', addr='buf', fix=False):
        """The C source (inline link programs), or a HIP module: the main kernels, or (``fix``) the fix-up kernels
        of the cells next to link-program walls."""
        if self.target != 'gpu':
            return emit(self.spec)
        mode = 'fix' if fix else 'main' if self.programs is not None else 'inline'
        return emit(dataclasses.replace(self.spec, idx=idx, addr=addr, mode=mode))

    # -- GPU ---------------------------------------------------------------------------------------
    def _gpu_fn(self, which, idx, addr, device):
        key = (which, idx, addr, device)
        fn = self._fns.get(key)
        if fn is None:
            from ..backends import hip_runtime as rt
            code = rt.compile_hip(self.source(idx, addr, fix=which.endswith('fix')), name='psad_lbm.hip')
            fn = self._fns[key] = rt.load_function(code, f'lbm_{which}', device)
        return fn

    def build(self):
        from ..backends import hip_runtime as rt
        if self.target == 'gpu':
            # both addressing modes of small arrays, and what arrays of 2³¹ − 1 elements and more take
            return [rt.compile_hip(self.source(i, a, f), name='psad_lbm.hip')
                    for i, a in (('int', 'buf'), ('int', 'ptr'), ('long long', 'ptr'))
                    for f in ((False, True) if self.programs is not None else (False,))]
        return self._cpu_fn('fwd')

    def _check_domain(self, arrays, mask, ids, ok=lambda a, itemsize: True):
        """What the kernels of both targets need: pdf arrays ``[*domain, Q]`` of one shape, the neighbour mask with
        walls and the wall ids with links (and neither without), both over the domain and ``ok``; returns the shape."""
        D, Q = self.stencil.D, self.stencil.Q
        shape = tuple(arrays[0].shape)
        for t in arrays:
            if tuple(t.shape) != shape or len(shape) != D + 1 or int(shape[D]) != Q:
                raise ValueError(f'pdf tensors must be [*domain, {Q}] of one shape, got {tuple(t.shape)}')
        if self.walls != (mask is not None):
            raise ValueError('the wall kernels need the neighbour mask (and the periodic ones none)')
        if (self.links is not None) != (ids is not None):
            raise ValueError('kernels with boundary links need the wall ids (and the others none)')
        for a, itemsize, msg in ((mask, 4, 'neighbour mask of shape {} does not match the domain {}'),
                                 (ids, 1, 'wall ids of shape {} do not match the domain {}')):
            if a is not None and (tuple(a.shape) != shape[:D] or not ok(a, itemsize)):
                raise ValueError(msg.format(tuple(a.shape), shape[:D]))
        return shape

    def _check(self, tensors, mask, ids=None):
        first = tensors[0]
        shape = self._check_domain(tensors, mask, ids, lambda a, itemsize: (
            a.is_contiguous() and a.dtype.itemsize == itemsize and a.device == first.device))
        if any(t.dtype != first.dtype or not t.is_cuda or t.device != first.device for t in tensors):
            raise ValueError('pdf tensors must share dtype and device')
        if min(shape[:-1]) < 2:
            raise ValueError('the periodic lattice needs at least 2 cells per axis')

    def tail_ptrs(self, which, mask, ids, force=None, dforce=None, scratch=None, omf=None, domf=None):
        """The pointers after the pdf arrays in the argument list of ``lbm_fwd`` / ``lbm_adj`` / ``lbm_adj_fix``: mask,
        ids, then force[, dforce], then the ω field[, its adjoint], then the second pass's scratch array (None: a slot
        patched per launch). Torch tensors, or numpy arrays on the C path."""
        ptrs = (_ptr(mask), _ptr(ids))
        if force is not None:
            ptrs += (_ptr(force),) + ((_ptr(dforce),) if which == 'adj' else ())
        if omf is not None:
            ptrs += (_ptr(omf),) + ((_ptr(domf),) if which == 'adj' else ())
        if which == 'adj' and self.link_pass:
            ptrs += (_ptr(scratch),)
        return ptrs

    @staticmethod
    def _reach(t):
        """Elements from the tensor's base to its last element (+1)."""
        return sum(abs(int(s)) * (int(n) - 1) for s, n in zip(t.stride(), t.shape)) + 1

    def _mode(self, tensors):
        """``(idx, addr)`` of a launch on these pdf tensors, by the largest reach among them: ``'buf'`` below 2³¹
        bytes (2 GiB) and ``'ptr'`` from there on (or with a negative stride, or ``PSAD_LBM_ADDR=ptr``); ``'int'``
        up to 2³¹ − 2 elements and ``'long long'`` from 2³¹ − 1."""
        reach = max(self._reach(t) for t in tensors)
        idx = 'int' if reach < 2 ** 31 - 1 else 'long long'
        esz = tensors[0].element_size()
        addr = 'buf' if reach * esz < 2 ** 31 and all(min(t.stride()) >= 0 for t in tensors) else 'ptr'
        if os.environ.get('PSAD_LBM_ADDR') == 'ptr':       # A/B of the addressing modes (probes)
            addr = 'ptr'
        return idx, addr

    def _launch_mode(self, tensors, force=None, dforce=None, omf=None, domf=None):
        """``(idx, addr)`` of a ``plan()`` launch: ``_mode`` of the pdf tensors; the force and the ω field (and
        their adjoints) are read through plain pointers with IDX offsets, so a far-reaching one widens ``idx`` alone."""
        idx, addr = self._mode(tensors)
        if max([self._reach(t) for t in (force, dforce, omf, domf) if t is not None], default=0) >= 2 ** 31 - 1:
            idx = 'long long'
        return idx, addr

    def _arg_format(self, idx, ntensors, nptr, nstrides, fix=False):
        """``(fmt, index of ω)`` of a ``plan()`` launch's argument buffer (``_pack``): ``nptr`` pointers, the
        extents, ``nstrides`` strides of type ``idx``, the ``ntensors`` pdf arrays' byte reaches, ω; the fix-up
        kernel's cell list and its length after them."""
        code = 'i' if idx == 'int' else 'q'
        fmt = 'Q' * nptr + 'iii' + code * nstrides + 'q' * ntensors + ('d' if self.ct == 'double' else 'f')
        return fmt + ('Qi' if fix else ''), len(fmt) - 1

    def _rho_format(self, idx):
        """``(fmt, index of the src slot or None)`` of a ``rho_plan()`` launch's argument buffer."""
        code = 'i' if idx == 'int' else 'q'
        fmt = 'QQQ' + 'iii' + code * 4
        if self.programs is None:
            return fmt, None
        return fmt + 'QQ' + code * 4, len(fmt)

    def _strides(self, arrays, force, omf=None):
        """The strides after the extents in every kernel's argument list: of each pdf array, then of the force field,
        then ``(s_z, s_y, s_x)`` of the ω field (2-D: ``s_z`` = 0)."""
        st = [n for a in list(arrays) + ([force] if force is not None else [])
              for n in lattice_strides(a, self.stencil.D)]
        if omf is not None:
            sw = [int(v) for v in (omf.stride() if hasattr(omf, 'stride') and callable(omf.stride) else
                                   [v // omf.itemsize for v in omf.strides])]
            st += [0] * (3 - len(sw)) + sw
        return st

    def _omega_check(self, shape, omf, domf, which, xp_tensor=True):
        """The per-cell relaxation rate (and, for the adjoint, its accumulated adjoint): ``[*domain]`` of the pdf
        dtype, ``domf`` with the strides of ``omf``; none without an ω field."""
        D = self.stencil.D
        need = [omf] + ([domf] if which == 'adj' else [])
        if not self.omega_field:
            if omf is not None or domf is not None:
                raise ValueError('these lattice kernels take no relaxation-rate field')
            return
        if any(t is None for t in need):
            raise ValueError('the ω-field lattice kernels need the relaxation-rate field'
                             f'{" and its adjoint" if which == "adj" else ""}')
        for t in need:
            if tuple(t.shape) != tuple(shape[:D]):
                raise ValueError(f'relaxation-rate field of shape {tuple(t.shape)}: expected {tuple(shape[:D])}')
            if (t.dtype != self.dtype) if not xp_tensor else (str(t.dtype).split('.')[-1] != self.dtype.name):
                raise ValueError(f'relaxation-rate field dtype {t.dtype}: expected {self.dtype}')
        if which == 'adj' and tuple(domf.stride() if xp_tensor else domf.strides) != \
                tuple(omf.stride() if xp_tensor else omf.strides):
            raise ValueError('the relaxation-rate adjoint must have the strides of the relaxation-rate field')

    def _force_check(self, shape, force, dforce, which, xp_tensor=True):
        """The per-cell force (and, for the adjoint, its accumulated adjoint): ``[*domain, D]`` of the pdf dtype,
        ``dforce`` with the strides of ``force``; none without a force field."""
        D = self.stencil.D
        need = [force] + ([dforce] if which == 'adj' else [])
        if not self.force_field:
            if force is not None or dforce is not None:
                raise ValueError('these lattice kernels take no force field')
            return
        if any(t is None for t in need):
            raise ValueError(f'the force-field lattice kernels need the force{" and its adjoint" if which == "adj" else ""}')
        for t in need:
            if tuple(t.shape) != tuple(shape[:D]) + (D,):
                raise ValueError(f'force field of shape {tuple(t.shape)}: expected {tuple(shape[:D]) + (D,)}')
            if (t.dtype != self.dtype) if not xp_tensor else (str(t.dtype).split('.')[-1] != self.dtype.name):
                raise ValueError(f'force field dtype {t.dtype}: expected {self.dtype}')
        if which == 'adj' and tuple(dforce.stride() if xp_tensor else dforce.strides) != \
                tuple(force.stride() if xp_tensor else force.strides):
            raise ValueError('the force adjoint must have the strides of the force')

    def plan(self, which, tensors, mask, omega, ids=None, force=None, dforce=None, fix=None, omf=None, domf=None):
        """The launch of ``which`` ('fwd' / 'adj') on tensors of these shapes, strides, dtype and device (with or
        without walls): a ``LaunchPlan`` whose pointer slots and relaxation rate are patched per launch — the
        time-step op launches T of them per apply. ω is not part of the key (a trained or scheduled rate reuses the
        plan); the plan is built with the first ω it sees. ``fix``: (cells,) — the fix-up kernel of ``which`` over
        the listed cells (int32 cell indices)."""
        key = (which, mask is not None) + tuple((tuple(t.shape), tuple(t.stride()), t.dtype, t.device)
                                                for t in tensors) + \
            ((tuple(force.shape), tuple(force.stride())) if force is not None else ()) + \
            (('omf', tuple(omf.shape), tuple(omf.stride())) if omf is not None else ()) + \
            ((fix[0].data_ptr(), int(fix[0].numel())) if fix is not None else ())
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        self._force_check(tuple(tensors[0].shape), force, dforce, which)
        self._omega_check(tuple(tensors[0].shape), omf, domf, which)
        self._check(tensors, mask, ids)
        if any(t is not None and (not t.is_cuda or t.device != tensors[0].device) for t in (omf, domf)):
            raise ValueError('the relaxation-rate field must be on the pdf tensors\' device')
        strides = self._strides(tensors, force, omf)
        idx, addr = self._launch_mode(tensors, force, dforce, omf, domf)
        dev = tensors[0].device.index
        fn = self._gpu_fn(which + ('_fix' if fix is not None else ''), idx, addr, dev)
        Z, Y, X = self._extent(tensors[0])
        nblocks = self._blocks(X, Y, Z) if fix is None else -(-int(fix[0].numel()) // FIX_BLOCK)
        reach = [self._reach(t) * t.element_size() for t in tensors]
        ptrs = [t.data_ptr() for t in tensors] + list(self.tail_ptrs(which, mask, ids, force, dforce, None, omf, domf))
        fmt, om_i = self._arg_format(idx, len(tensors), len(ptrs), len(strides), fix is not None)
        vals = [*ptrs, Z, Y, X, *strides, *reach, float(omega)]
        if fix is not None:
            # the fix-up kernel: the cell list and its length after the main kernel's arguments
            vals += [fix[0].data_ptr(), int(fix[0].numel())]
        args = _pack(fmt, *vals)
        plan = self._plans[key] = LaunchPlan(fn, nblocks, args, len(ptrs), dev, _offset(fmt, om_i), fmt[om_i])
        if fix is not None:
            plan.block = FIX_BLOCK
        return plan

    def fix_launch(self, which, tensors, mask, omega, ids, force, dforce, cells, stream, omf=None, domf=None):
        """The fix-up launch after a main adjoint launch on ``tensors`` (HIP with link programs; nothing for the
        forward, which runs them inline, or when no cell is listed): the listed cells' adjoint with their programs'
        Jacobian terms, added atomically into the entries the main launch left zeroed (no second fix-up launch)."""
        if which != 'adj' or self.programs is None or self.target != 'gpu' or cells is None or \
                int(cells.numel()) == 0:
            return
        plan = self.plan(which, tensors, mask, omega, ids, force, dforce, fix=(cells,), omf=omf, domf=domf)
        rho = self.rho_buffer(tensors[0]) if self.link_pass else None
        plan(tuple(t.data_ptr() for t in tensors) + self.tail_ptrs(which, mask, ids, force, dforce, rho, omf, domf),
             stream, omega)

    def _scratch_shape(self, domain):
        """Of the second adjoint pass's scratch array: one value per cell (density-weighted links); with inline link
        programs (the C target) Q per cell and the density term's slot after them. (HIP: link programs run in the
        fix-up kernels, so the density pass alone uses it — one slot.)"""
        inline = self.programs is not None and self.target != 'gpu'
        return ((self.stencil.Q + int(self.rho_links),) if inline else ()) + tuple(domain)

    def rho_buffer(self, t):
        """The per-cell scratch array of the second adjoint pass (one per domain and device, reused: stream-ordered)."""
        import torch
        key = (tuple(int(n) for n in t.shape[:self.stencil.D]), t.device, t.dtype)
        b = self._rho_bufs.get(key)
        if b is None:
            b = self._rho_bufs[key] = torch.empty(self._scratch_shape(key[0]), dtype=t.dtype, device=t.device)
        return b

    def rho_plan(self, out, mask, rho, src=None, ids=None):
        """The second pass of the adjoint (``lbm_adj_rho``: every component of a cell next to a density-weighted
        wall gets the cell's Σ_j βρ_j v_j added; with link programs, component k of a cell next to a program wall
        gets Σ_j J_jk v_j, the Jacobians evaluated at the cell's own pdfs in ``src``) on ``out``'s shape and strides.
        The plan's pointer slots: out, mask, scratch (+ src, ids with link programs)."""
        key = ('rho', tuple(out.shape), tuple(out.stride()), out.dtype, out.device) + \
            ((tuple(src.stride()),) if self.programs is not None else ())
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        tensors = [out] + ([src] if self.programs is not None else [])
        idx, addr = self._mode(tensors)
        dev = out.device.index
        fn = self._gpu_fn('adj_rho', idx, addr, dev)
        Z, Y, X = self._extent(out)
        fmt, extra_i = self._rho_format(idx)
        vals = [out.data_ptr(), mask.data_ptr(), rho.data_ptr(), Z, Y, X, *lattice_strides(out, self.stencil.D)]
        if self.programs is not None:
            # the src / ids slots of the inline (C-style) second pass; the HIP ``lbm_adj_rho`` of a lattice with
            # programs does not take them (its programs run in the fix-up kernel) and ignores the extra bytes
            vals += [src.data_ptr(), ids.data_ptr(), *lattice_strides(src, self.stencil.D)]
        plan = self._plans[key] = LaunchPlan(fn, self._blocks(X, Y, Z), _pack(fmt, *vals), 3, dev, None, None)
        if self.programs is not None:
            plan.extra = _offset(fmt, extra_i)            # the src / ids slots, patched per launch
        return plan

    def forward(self, src, dst, omega, mask=None, stream=None, ids=None, force=None, cells=None, omf=None):
        """``dst = stream-pull-collide(src)`` (torch tensors ``[*domain, q]``, any strides; ``force``: the per-cell
        force ``[*domain, D]`` of force-field kernels; ``omf``: the per-cell relaxation rate ``[*domain]`` of ω-field
        kernels, which ignore ``omega``)."""
        if self.target != 'gpu':
            return self._cpu('fwd', [src, dst], omega, mask, ids, force, omf=omf)
        st = _stream(stream, src)
        self.plan('fwd', [src, dst], mask, omega, ids, force, omf=omf)(
            (src.data_ptr(), dst.data_ptr()) + self.tail_ptrs('fwd', mask, ids, force, omf=omf), st, omega)

    def adjoint(self, src, g, out, omega, mask=None, stream=None, ids=None, force=None, dforce=None, cells=None,
                omf=None, domf=None):
        """``out = (∂ step / ∂ src)ᵀ g`` at the state ``src``; force-field kernels also ADD ``(∂ step / ∂ F)ᵀ g`` to
        ``dforce``, ω-field kernels ``(∂ step / ∂ ω)ᵀ g`` to ``domf``."""
        if self.target != 'gpu':
            return self._cpu('adj', [src, g, out], omega, mask, ids, force, dforce, omf, domf)
        st = _stream(stream, src)
        rho = self.rho_buffer(src) if self.link_pass else None
        self.plan('adj', [src, g, out], mask, omega, ids, force, dforce, omf=omf, domf=domf)(
            (src.data_ptr(), g.data_ptr(), out.data_ptr()) +
            self.tail_ptrs('adj', mask, ids, force, dforce, rho, omf, domf), st, omega)
        self.fix_launch('adj', [src, g, out], mask, omega, ids, force, dforce, cells, st, omf, domf)
        if rho is not None:
            self.rho_pass(out, mask, rho, src, ids, st)

    def rho_pass(self, out, mask, rho, src, ids, stream):
        """Launch the adjoint's second pass (``rho_plan``) for this launch's ``out`` / ``src``."""
        plan = self.rho_plan(out, mask, rho, src, ids)
        plan((out.data_ptr(), mask.data_ptr(), rho.data_ptr()), stream,
             extra=(src.data_ptr(), ids.data_ptr()) if self.programs is not None else None)

    def _extent(self, t):
        shape = [int(n) for n in t.shape[:self.stencil.D]]
        return [1] + shape if self.stencil.D == 2 else shape

    @staticmethod
    def _blocks(X, Y, Z):
        """One block per 256 consecutive cells (cell indices are 32-bit in the kernel)."""
        if X * Y * Z + 255 >= 2 ** 32:
            raise ValueError('lattice of 2^32 cells or more: too large for one launch')
        return -(-(X * Y * Z) // 256)

    # -- CPU ---------------------------------------------------------------------------------------
    def _cpu_fn(self, which):
        fn = self._fns.get(which)
        if fn is None:
            from ..backends.cpu_kernel import compile_c
            fn = self._fns[which] = compile_c(self.source(), f'lbm_{which}', openmp=True)
        return fn

    def _cpu(self, which, arrays, omega, mask, ids=None, force=None, dforce=None, omf=None, domf=None):
        arrays = [np.asarray(a) for a in arrays]
        for a in arrays:
            if a.dtype != self.dtype:
                raise TypeError(f'pdf arrays must be {self.dtype}, got {a.dtype}')
        D = self.stencil.D
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint32)
        idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint8)
        shape = self._check_domain(arrays, m, idv)
        self._force_check(shape, force, dforce, which, xp_tensor=False)
        self._omega_check(shape, omf, domf, which, xp_tensor=False)
        fn = self._cpu_fn(which)
        strides = self._strides(arrays, force, omf)
        # the second pass's scratch (both passes in one call)
        rho = np.empty(self._scratch_shape(shape[:D]), self.dtype) if which == 'adj' and self.link_pass else None
        ptrs = [a.ctypes.data for a in arrays] + list(self.tail_ptrs(which, m, idv, force, dforce, rho, omf, domf))
        ext = list(shape[:D]) if D == 3 else [1] + list(shape[:D])
        P = (ctypes.c_void_p * len(ptrs))(*ptrs)
        N = (ctypes.c_longlong * 3)(*ext)
        S = (ctypes.c_longlong * len(strides))(*strides)
        B = (ctypes.c_longlong * 1)(0)
        Dv = (ctypes.c_double * 1)(float(omega))
        fn(P, N, S, B, Dv)


class LaunchPlan:
    """One lattice kernel launch with its argument buffer; ``plan(ptrs, stream, omega)`` patches the leading pointer
    slots (the pdf arrays, then the neighbour mask) and the relaxation rate, and launches on the plan's device
    (made current for the launch when it is not: the function handle belongs to that device's module)."""
    __slots__ = ('fn', 'nblocks', 'template', 'fmt', 'device', 'om_off', 'om_fmt', 'extra', 'block')

    def __init__(self, fn, nblocks, template, nptr, device, om_off, om_code):
        self.fn, self.nblocks, self.template, self.fmt = fn, nblocks, template, f'<{nptr}Q'
        self.device, self.om_off, self.om_fmt = device, om_off, None if om_code is None else '<' + om_code
        self.extra = None              # byte offset of two more pointer slots patched per launch (second pass)
        self.block = 256

    def __call__(self, ptrs, stream, omega=None, extra=None):
        from ..backends import hip_runtime as rt
        buf = bytearray(self.template)
        struct.pack_into(self.fmt, buf, 0, *ptrs)
        if extra is not None:
            struct.pack_into('<2Q', buf, self.extra, *extra)
        if omega is not None and self.om_off is not None:
            struct.pack_into(self.om_fmt, buf, self.om_off, float(omega))
        import torch
        if self.device is not None and self.device != torch.cuda.current_device():
            with torch.cuda.device(self.device):
                rt.launch(self.fn, (self.nblocks,), (self.block,), bytes(buf), stream)
        else:
            rt.launch(self.fn, (self.nblocks,), (self.block,), bytes(buf), stream)


def _ptr(a):
    """Address of a torch tensor or a numpy array (0 for None)."""
    return 0 if a is None else a.data_ptr() if hasattr(a, 'data_ptr') else a.ctypes.data


def _stream(stream, t):
    if stream is not None:
        return stream
    import torch
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _offset(fmt, i):
    """Byte offset of argument ``i`` in ``_pack(fmt, ...)``."""
    off = 0
    for j, c in enumerate(fmt):
        size = struct.calcsize(c)
        off += (-off) % size
        if j == i:
            return off
        off += size
    raise IndexError(i)


def _pack(fmt, *vals):
    """Kernel arguments at natural alignment (``HIP_LAUNCH_PARAM_BUFFER``)."""
    out, off = b'', 0
    for c, v in zip(fmt, vals):
        size = struct.calcsize(c)
        pad = (-off) % size
        out += b'\0' * pad + struct.pack('<' + c, v)
        off += pad + size
    return out + b'\0' * ((-off) % 8)
