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
host side: masks and cell lists, compiling, argument buffers and launches. Every argument buffer is laid out by the
printer's own table of the kernel's arguments (``_lattice_source.args.kernel_args``) and filled by name. The per-cell
fields of a launch (force, relaxation rate, solid fraction: the rows of ``_lattice_source.fields.CELL_FIELDS``) travel
as one bundle ``{kind: (array, adjoint or None)}`` (``field_pair``); only ``forward`` / ``adjoint`` take them as keywords.
"""
import ctypes
import dataclasses
import os
import struct

import numpy as np

from ._lattice_source import FIX_BIT, FIX_BLOCK, SELF_BIT  # noqa: F401 (the bits: re-exported)
from ._lattice_source import ARRAYS, CELL_FIELDS, LatticeSource, emit, kernel_args, link_programs, struct_format
from ._lattice_source.args import CELLS, EXTENT, KERNELS, POINTER, RATE, REACH, STRIDE

__all__ = ['LatticeKernels', 'LaunchPlan', 'lattice_strides', 'row_interleaved_empty', 'neighbour_mask',
           'addressing_mode']


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
    for wid, wall in enumerate(link_programs(programs)):
        for d, pg in enumerate(wall or ()):
            if pg is None or not pg.reads:
                continue
            # the fluid cells x whose link of direction d ends in a wall cell of this id: x + c_d
            src = fluid & np.roll(f == wid, tuple(-int(v) for v in stencil.directions[d]), axis=axes)
            for o in pg.reads:
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


def _element_strides(t):
    """Strides in elements of a torch tensor or a numpy array."""
    return [int(s) for s in (t.stride() if hasattr(t, 'stride') and callable(t.stride) else
                             [s // t.itemsize for s in t.strides])]


def lattice_strides(t, D):
    """``(s_q, s_z, s_y, s_x)`` in elements of a pdf tensor ``[*spatial, q]`` (2-D: ``s_z`` = 0)."""
    st = _element_strides(t)
    return (st[D],) + (0,) * (3 - D) + tuple(st[:D])


def field_pair(fields, kind):
    """``(array, adjoint)`` of the per-cell field ``kind`` in a launch's bundle ``fields`` (``{kind: (array, adjoint or
    None)}`` over the kinds of ``CELL_FIELDS``, or None for no field at all): ``(None, None)`` for one not given."""
    return (fields or {}).get(kind, (None, None))


def _stride_values(ops, D):
    """name → value of every stride argument the operands ``ops`` give: ``{p}_{q,z,y,x}`` of the pdf arrays and the
    per-cell fields' by their rows of ``CELL_FIELDS`` (``f_{c,z,y,x}``, ``w_{z,y,x}``, ``p_{z,y,x}``; 2-D: the z strides
    are 0)."""
    v = {}
    for p, name in ARRAYS.items():
        if ops.get(name) is not None:
            v.update(zip((f'{p}_q', f'{p}_z', f'{p}_y', f'{p}_x'), lattice_strides(ops[name], D)))
    for f in CELL_FIELDS:
        t = ops.get(f.operand)
        if t is not None:
            st = _element_strides(t)
            v.update(zip(f.strides, lattice_strides(t, D) if f.vector else [0] * (3 - len(st)) + st))
    # the density / velocity outputs and their seeds (one set of strides: the seeds have the outputs' layout)
    rho = ops.get('rho_out') if ops.get('rho_out') is not None else ops.get('drho')
    vel = ops.get('vel_out') if ops.get('vel_out') is not None else ops.get('dvel')
    if rho is not None:
        sr = _element_strides(rho)
        v.update(zip(('r_z', 'r_y', 'r_x'), [0] * (3 - len(sr)) + sr))
        v.update(zip(('v_c', 'v_z', 'v_y', 'v_x'), lattice_strides(vel, D)))
    return v


def row_interleaved_empty(domain, Q, dtype, device):
    """An uninitialised pdf tensor ``[*domain, Q]`` in the row-interleaved layout ``[z][y][q][x]`` (each lattice
    row's Q components one contiguous block) — the time-step op's internal states."""
    import torch
    dims = list(domain)
    base = torch.empty(dims[:-1] + [Q, dims[-1]], dtype=dtype, device=device)
    return base.transpose(-1, -2)


def _reach(t):
    """Elements from the tensor's base to its last element (+1)."""
    return sum(abs(int(s)) * (int(n) - 1) for s, n in zip(t.stride(), t.shape)) + 1


def addressing_mode(tensors):
    """``(idx, addr)`` of a launch on these pdf tensors, by the largest reach among them: ``'buf'`` below 2³¹
    bytes (2 GiB) and ``'ptr'`` from there on (or with a negative stride, or ``PSAD_LBM_ADDR=ptr``); ``'int'``
    up to 2³¹ − 2 elements and ``'long long'`` from 2³¹ − 1. (The lattice kernels' and the boundary-force kernels'.)"""
    reach = max(_reach(t) for t in tensors)
    idx = 'int' if reach < 2 ** 31 - 1 else 'long long'
    esz = tensors[0].element_size()
    addr = 'buf' if reach * esz < 2 ** 31 and all(min(t.stride()) >= 0 for t in tensors) else 'ptr'
    if os.environ.get('PSAD_LBM_ADDR') == 'ptr':       # A/B of the addressing modes (probes)
        addr = 'ptr'
    return idx, addr


class LatticeKernels:
    """Compiled forward / adjoint lattice kernels of one (stencil, compressible, dtype, walls, links, target).
    ``mask`` arguments are the cells' neighbour masks (``neighbour_mask``), ``None`` without walls; ``ids`` the
    cells' wall ids (the ``uint8`` flag array, C order) when ``links`` is given (walls other than plain
    bounce-back)."""

    def __init__(self, stencil, compressible, dtype, walls, target, links=None, force_model=None, force=None,
                 force_field=False, trt=None, programs=None, mrt=None, *, omega_field=False, zero_centered=False,
                 smagorinsky=None, solid_field=False):
        self.stencil = stencil
        # the Smagorinsky constant C_s (None: no subgrid model): a constant of the emitted source, so of every cache
        # key made from it
        self.smagorinsky = None if smagorinsky is None else float(smagorinsky)
        # the state arrays hold f_i − w_i (``LatticeSource.zero_centered``); the adjoint arrays are not shifted
        self.zero_centered = bool(zero_centered)
        # ω read per cell from a scalar field ``[*domain]``, its adjoint accumulated by the adjoint launches
        self.omega_field = bool(omega_field)
        # the solid fraction σ read per cell from a scalar field ``[*domain]`` (partial bounce-back), its adjoint
        # accumulated by the adjoint launches
        self.solid_field = bool(solid_field)
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
            smagorinsky=self.smagorinsky, solid_field=self.solid_field)
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
        # every kernel's arguments as the printer declares them (the same for every index type and addressing
        # mode), and the names of the pointers among them, which a launch patches (``lbm_adj_fix``: ``lbm_adj``'s)
        self._tables = {k: kernel_args(self._spec(fix=k == 'adj_fix'), k) for k in KERNELS}
        self._ptr_names = {k: tuple(a.name for a in t if a.kind == POINTER) for k, t in self._tables.items()}
        # ... and of the variant with the density / velocity outputs (``macro``: a module of its own, launched for
        # the observed steps only)
        self._mtables = {k: kernel_args(self._spec(fix=k == 'adj_fix', macro=True), k) for k in KERNELS}
        self._mptr_names = {k: tuple(a.name for a in t if a.kind == POINTER) for k, t in self._mtables.items()}

    def _spec(self, idx='int', addr='buf', fix=False, macro=False):
        """What ``source`` prints: the C spec (inline link programs), or of a HIP module: the main kernels, or
        (``fix``) the fix-up kernels of the cells next to link-program walls. ``macro``: the variant that writes ρ
        and u of the stored state and takes their adjoint seeds (``LatticeSource.macroscopic``)."""
        if self.target != 'gpu':
            return dataclasses.replace(self.spec, macroscopic=True) if macro else self.spec
        mode = 'fix' if fix else 'main' if self.programs is not None else 'inline'
        return dataclasses.replace(self.spec, idx=idx, addr=addr, mode=mode, macroscopic=bool(macro))

    def source(self, idx='int', addr='buf', fix=False, macro=False):
        return emit(self._spec(idx, addr, fix, macro))

    def table(self, kernel, macro=False):
        """The arguments of ``lbm_{kernel}`` ('fwd' / 'adj' / 'adj_rho' / 'adj_fix')."""
        return (self._mtables if macro else self._tables)[kernel]

    def table_pointer_names(self, kernel, macro=False):
        """The names of the pointer arguments of ``lbm_{kernel}``, in the table's order (``lbm_adj_fix``: ``lbm_adj``'s
        and the cell list)."""
        return (self._mptr_names if macro else self._ptr_names)[kernel]

    def arg_format(self, kernel, idx):
        """The ``struct`` codes of ``lbm_{kernel}``'s argument buffer (``_pack``) with strides of type ``idx``."""
        return struct_format(self.table(kernel), idx, self.ct)

    # -- GPU ---------------------------------------------------------------------------------------
    def _gpu_fn(self, which, idx, addr, device, macro=False):
        key = (which, idx, addr, device) + (('macro',) if macro else ())
        fn = self._fns.get(key)
        if fn is None:
            from ..backends import hip_runtime as rt
            code = rt.compile_hip(self.source(idx, addr, fix=which.endswith('fix'), macro=macro), name='psad_lbm.hip')
            fn = self._fns[key] = rt.load_function(code, f'lbm_{which}', device)
        return fn

    def build(self, macro=False):
        from ..backends import hip_runtime as rt
        if self.target == 'gpu':
            # both addressing modes of small arrays, and what arrays of 2³¹ − 1 elements and more take
            return [rt.compile_hip(self.source(i, a, f, macro), name='psad_lbm.hip')
                    for i, a in (('int', 'buf'), ('int', 'ptr'), ('long long', 'ptr'))
                    for f in ((False, True) if self.programs is not None else (False,))]
        return self._cpu_fn('fwd', macro)

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

    @staticmethod
    def operands(tensors, mask, ids, fields=None, scratch=None, macro=None):
        """Argument name → operand (torch tensors, or numpy arrays on the C path; None: not given) of ``lbm_fwd``
        (``tensors``: src, dst) or ``lbm_adj`` / ``lbm_adj_fix`` (src, g, out). ``fields``: the launch's per-cell fields
        (``field_pair``), under the names their rows of ``CELL_FIELDS`` print. ``macro``: None, or by name the arrays
        of the density / velocity variant (``rho_out``, ``vel_out``, ``drho``, ``dvel``)."""
        ops = dict(zip(('src', 'dst') if len(tensors) == 2 else ('src', 'g', 'out'), tensors), nbmask=mask,
                   wallid=ids, rho_adj=scratch, **(macro or {}))
        for f in CELL_FIELDS if fields else ():
            ops[f.operand], ops[f.adjoint] = field_pair(fields, f.kind)
        return ops

    def pointers(self, kernel, ops, macro=False):
        """The pointer slots a launch of ``lbm_{kernel}`` patches, in the table's order, from the operands ``ops``
        (0 for one not given)."""
        return tuple(_ptr(ops.get(n)) for n in (self._mptr_names if macro else self._ptr_names)[kernel])

    def _macro_check(self, which, shape, macro, xp_tensor=True):
        """The arrays of the density / velocity variant, by name: the forward's ``rho_out`` ``[*domain]`` and ``vel_out``
        ``[*domain, D]``, the adjoint's seeds ``drho`` / ``dvel`` (and, compressible, the recorded outputs, with the
        seeds' strides), all of the compute type; returns them in the table's order."""
        D = self.stencil.D
        names = [a.name for a in self._mtables[which] if a.group == 'macro' and a.kind == POINTER]
        dt = 'float64' if self.ct == 'double' else 'float32'
        for n in names:
            t = macro.get(n)
            if t is None:
                raise ValueError(f'the density / velocity lattice kernels need {", ".join(names)}: {n} is missing')
            want = tuple(shape[:D]) + ((D,) if n in ('vel_out', 'dvel') else ())
            if tuple(t.shape) != want:
                raise ValueError(f'{n} of shape {tuple(t.shape)}: expected {want}')
            if str(t.dtype).split('.')[-1] != dt:
                raise ValueError(f'{n} dtype {t.dtype}: expected {dt}')
        st = [tuple(macro[n].stride() if xp_tensor else macro[n].strides) for n in names]
        if which == 'adj' and len(names) == 4 and (st[0] != st[2] or st[1] != st[3]):
            raise ValueError('the density / velocity seeds must have the strides of the recorded outputs')
        return [macro[n] for n in names]

    def _values(self, table, ops, omega=None):
        """The value of every argument of ``table`` from the operands ``ops`` (a pointer not given: 0, a slot patched
        per launch)."""
        strides = _stride_values(ops, self.stencil.D)
        extent = dict(zip('ZYX', self._extent(ops[table[0].name])))
        vals = []
        for a in table:
            if a.kind in (POINTER, CELLS):
                vals.append(_ptr(ops.get(a.name)))
            elif a.kind in (EXTENT, STRIDE):
                vals.append(extent[a.name] if a.kind == EXTENT else strides[a.name])
            elif a.kind == REACH:
                t = ops[ARRAYS[a.name[0]]]
                vals.append(self._reach(t) * t.element_size())
            else:
                vals.append(float(omega) if a.kind == RATE else int(ops['cells'].numel()))
        return vals

    _reach = staticmethod(_reach)

    def _mode(self, tensors):
        """``(idx, addr)`` of a launch on these pdf tensors, by the largest reach among them: ``'buf'`` below 2³¹
        bytes (2 GiB) and ``'ptr'`` from there on (or with a negative stride, or ``PSAD_LBM_ADDR=ptr``); ``'int'``
        up to 2³¹ − 2 elements and ``'long long'`` from 2³¹ − 1 (``addressing_mode``)."""
        return addressing_mode(tensors)

    def _launch_mode(self, tensors, fields=None, more=()):
        """``(idx, addr)`` of a ``plan()`` launch: ``_mode`` of the pdf tensors; the per-cell fields and their adjoints
        (``fields``) and the arrays ``more`` are read through plain pointers with IDX offsets, so a far-reaching one
        widens ``idx`` alone."""
        idx, addr = self._mode(tensors)
        plain = [t for f in CELL_FIELDS for t in field_pair(fields, f.kind)] + list(more)
        if max([self._reach(t) for t in plain if t is not None], default=0) >= 2 ** 31 - 1:
            idx = 'long long'
        return idx, addr

    def _field_check(self, shape, fields, which, xp_tensor=True):
        """The per-cell fields of a launch, each by its row of ``CELL_FIELDS`` — ``[*domain, D]`` or ``[*domain]`` —
        and, for the adjoint kernel, its accumulated adjoint: both of the pdf dtype, ``adjoint`` with the strides of
        ``field``; none where the kernels take no such field."""
        D = self.stencil.D
        for f in CELL_FIELDS:
            field, adjoint = field_pair(fields, f.kind)
            want = tuple(shape[:D]) + ((D,) if f.vector else ())
            need = [field] + ([adjoint] if which == 'adj' else [])
            if not getattr(self.spec, f.flag):
                if field is not None or adjoint is not None:
                    raise ValueError(f'these lattice kernels take no {f.what}')
                continue
            if any(t is None for t in need):
                raise ValueError(f'the {f.kernels} lattice kernels need the {f.name}'
                                 f'{" and its adjoint" if which == "adj" else ""}')
            for t in need:
                if tuple(t.shape) != want:
                    raise ValueError(f'{f.what} of shape {tuple(t.shape)}: expected {want}')
                if (t.dtype != self.dtype) if not xp_tensor else (str(t.dtype).split('.')[-1] != self.dtype.name):
                    raise ValueError(f'{f.what} dtype {t.dtype}: expected {self.dtype}')
            if which == 'adj' and tuple(adjoint.stride() if xp_tensor else adjoint.strides) != \
                    tuple(field.stride() if xp_tensor else field.strides):
                raise ValueError(f'the {f.short} adjoint must have the strides of the {f.name}')

    def plan(self, which, tensors, mask, omega, ids=None, fields=None, fix=None, macro=None):
        """The launch of ``which`` ('fwd' / 'adj') on tensors of these shapes, strides, dtype and device (with or
        without walls): a ``LaunchPlan`` whose pointer slots and relaxation rate are patched per launch — the
        time-step op launches T of them per apply. ω is not part of the key (a trained or scheduled rate reuses the
        plan); the plan is built with the first ω it sees. ``fix``: (cells,) — the fix-up kernel of ``which`` over
        the listed cells (int32 cell indices). ``fields``: the launch's per-cell fields (``field_pair``). ``macro``: the
        arrays of the density / velocity variant (``operands``), whose pointers every launch patches too."""
        key = (which, mask is not None) + tuple((tuple(t.shape), tuple(t.stride()), t.dtype, t.device)
                                                for t in tensors) + \
            tuple((k, tuple(t.shape), tuple(t.stride())) for k, (t, _) in (fields or {}).items() if t is not None) + \
            ((fix[0].data_ptr(), int(fix[0].numel())) if fix is not None else ()) + \
            (('macro',) + tuple((n, tuple(t.stride())) for n, t in sorted(macro.items()) if t is not None)
             if macro else ())
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        marr = self._macro_check(which, tuple(tensors[0].shape), macro) if macro else []
        if any(not t.is_cuda or t.device != tensors[0].device for t in marr):
            raise ValueError('the density / velocity arrays must be on the pdf tensors\' device')
        self._field_check(tuple(tensors[0].shape), fields, which)
        self._check(tensors, mask, ids)
        for f in CELL_FIELDS:
            if any(t is not None and (not t.is_cuda or t.device != tensors[0].device)
                   for t in field_pair(fields, f.kind)):
                raise ValueError(f'the {f.what} must be on the pdf tensors\' device')
        idx, addr = self._launch_mode(tensors, fields, marr)
        dev = tensors[0].device.index
        # (the fix-up kernel: the cell list and its length after the main kernel's arguments)
        kernel = which + ('_fix' if fix is not None else '')
        fn = self._gpu_fn(kernel, idx, addr, dev, bool(macro))
        Z, Y, X = self._extent(tensors[0])
        nblocks = self._blocks(X, Y, Z) if fix is None else -(-int(fix[0].numel()) // FIX_BLOCK)
        table = self.table(kernel, bool(macro))
        fmt = struct_format(table, idx, self.ct)
        ops = dict(self.operands(tensors, mask, ids, fields, macro=macro), cells=fix[0] if fix else None)
        om_i = [a.kind for a in table].index(RATE)
        nptr = len((self._mptr_names if macro else self._ptr_names)[which])
        plan = self._plans[key] = LaunchPlan(fn, nblocks, _pack(fmt, *self._values(table, ops, omega)),
                                             nptr, dev, _offset(fmt, om_i), fmt[om_i])
        if fix is not None:
            plan.block = FIX_BLOCK
        return plan

    def fix_launch(self, which, tensors, mask, omega, ids, fields, cells, stream, macro=None):
        """The fix-up launch after a main adjoint launch on ``tensors`` (HIP with link programs; nothing for the
        forward, which runs them inline, or when no cell is listed): the listed cells' adjoint with their programs'
        Jacobian terms, added atomically into the entries the main launch left zeroed (no second fix-up launch)."""
        if which != 'adj' or self.programs is None or self.target != 'gpu' or cells is None or \
                int(cells.numel()) == 0:
            return
        plan = self.plan(which, tensors, mask, omega, ids, fields, fix=(cells,), macro=macro)
        rho = self.rho_buffer(tensors[0]) if self.link_pass else None
        plan(self.pointers(which, self.operands(tensors, mask, ids, fields, rho, macro), bool(macro)), stream, omega)

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

    def rho_plan(self, out, mask, rho):
        """The second pass of the adjoint on the HIP target (``lbm_adj_rho``: every component of a cell next to a
        density-weighted wall gets the cell's Σ_j βρ_j v_j added; link programs run in the fix-up kernel there) on
        ``out``'s shape and strides. The plan's pointer slots: out, mask, scratch."""
        key = ('rho', tuple(out.shape), tuple(out.stride()), out.dtype, out.device)
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        idx, addr = self._mode([out])
        dev = out.device.index
        fn = self._gpu_fn('adj_rho', idx, addr, dev)
        table = self.table('adj_rho')
        args = _pack(struct_format(table, idx, self.ct),
                     *self._values(table, dict(out=out, nbmask=mask, rho_adj=rho)))
        plan = self._plans[key] = LaunchPlan(fn, self._blocks(*reversed(self._extent(out))), args,
                                             len(self._ptr_names['adj_rho']), dev, None, None)
        return plan

    def forward(self, src, dst, omega, mask=None, stream=None, ids=None, force=None, cells=None, omf=None,
                rho_out=None, vel_out=None, sof=None):
        """``dst = stream-pull-collide(src)`` (torch tensors ``[*domain, q]``, any strides; ``force``: the per-cell
        force ``[*domain, D]`` of force-field kernels; ``omf``: the per-cell relaxation rate ``[*domain]`` of ω-field
        kernels, which ignore ``omega``; ``sof``: the per-cell solid fraction ``[*domain]`` of σ-field kernels).
        ``rho_out`` / ``vel_out`` (both or neither; the compute type, ``[*domain]``
        and ``[*domain, D]``, any strides): also written, the density and the velocity of ``dst`` — 0 in obstacle
        cells — by the kernels' density / velocity variant."""
        macro = None if rho_out is None and vel_out is None else dict(rho_out=rho_out, vel_out=vel_out)
        self.run('fwd', [src, dst], omega, mask, ids, dict(force=(force, None), omega=(omf, None), solid=(sof, None)),
                 macro, cells, stream)

    def adjoint(self, src, g, out, omega, mask=None, stream=None, ids=None, force=None, dforce=None, cells=None,
                omf=None, domf=None, rho_out=None, vel_out=None, drho=None, dvel=None, sof=None, dsof=None):
        """``out = (∂ step / ∂ src)ᵀ g`` at the state ``src``; force-field kernels also ADD ``(∂ step / ∂ F)ᵀ g`` to
        ``dforce``, ω-field kernels ``(∂ step / ∂ ω)ᵀ g`` to ``domf``, σ-field kernels ``(∂ step / ∂ σ)ᵀ g`` to ``dsof``.
        ``drho`` / ``dvel`` (both or neither): the
        adjoint seeds of the density and the velocity of this step's output, added to ``g`` in the cell (with the
        recorded ``rho_out`` / ``vel_out`` of that step, which a compressible rule reads)."""
        macro = None if drho is None and dvel is None else dict(rho_out=rho_out, vel_out=vel_out, drho=drho, dvel=dvel)
        self.run('adj', [src, g, out], omega, mask, ids,
                 dict(force=(force, dforce), omega=(omf, domf), solid=(sof, dsof)), macro, cells, stream)

    def run(self, which, tensors, omega, mask=None, ids=None, fields=None, macro=None, cells=None, stream=None):
        """One launch of ``which`` — 'fwd' on (src, dst), 'adj' on (src, g, out) with its fix-up launch and second pass
        — what ``forward`` / ``adjoint`` do, which only turn their keywords into the bundle ``fields`` (``field_pair``)
        and the by-name arrays ``macro`` (``operands``)."""
        if self.target != 'gpu':
            return self._cpu(which, tensors, omega, mask, ids, fields, macro)
        st = _stream(stream, tensors[0])
        rho = self.rho_buffer(tensors[0]) if which == 'adj' and self.link_pass else None
        self.plan(which, tensors, mask, omega, ids, fields, macro=macro)(
            self.pointers(which, self.operands(tensors, mask, ids, fields, rho, macro), bool(macro)), st, omega)
        self.fix_launch(which, tensors, mask, omega, ids, fields, cells, st, macro)
        if rho is not None:
            self.rho_pass(tensors[2], mask, rho, st)

    def rho_pass(self, out, mask, rho, stream):
        """Launch the adjoint's second pass (``rho_plan``) for this launch's ``out``."""
        self.rho_plan(out, mask, rho)(self.pointers('adj_rho', dict(out=out, nbmask=mask, rho_adj=rho)), stream)

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
    def _cpu_fn(self, which, macro=False):
        key = (which, 'macro') if macro else which
        fn = self._fns.get(key)
        if fn is None:
            from ..backends.cpu_kernel import compile_c
            fn = self._fns[key] = compile_c(self.source(macro=macro), f'lbm_{which}', openmp=True)
        return fn

    def _cpu(self, which, arrays, omega, mask, ids=None, fields=None, macro=None):
        arrays = [np.asarray(a) for a in arrays]
        for a in arrays:
            if a.dtype != self.dtype:
                raise TypeError(f'pdf arrays must be {self.dtype}, got {a.dtype}')
        D = self.stencil.D
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint32)
        idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint8)
        shape = self._check_domain(arrays, m, idv)
        self._field_check(shape, fields, which, xp_tensor=False)
        if macro:
            self._macro_check(which, shape, macro, xp_tensor=False)
        fn = self._cpu_fn(which, bool(macro))
        # the second pass's scratch (both passes in one call)
        rho = np.empty(self._scratch_shape(shape[:D]), self.dtype) if which == 'adj' and self.link_pass else None
        # ``P`` / ``S``: the table's pointers and strides, each in the table's order
        ops = self.operands(arrays, m, idv, fields, rho, macro)
        ptrs = self.pointers(which, ops, bool(macro))
        named = _stride_values(ops, D)
        strides = [named[a.name] for a in self.table(which, bool(macro)) if a.kind == STRIDE]
        ext = list(shape[:D]) if D == 3 else [1] + list(shape[:D])
        P = (ctypes.c_void_p * len(ptrs))(*ptrs)
        N = (ctypes.c_longlong * 3)(*ext)
        S = (ctypes.c_longlong * len(strides))(*strides)
        B = (ctypes.c_longlong * 1)(0)
        Dv = (ctypes.c_double * 1)(float(omega))
        fn(P, N, S, B, Dv)


class LaunchPlan:
    """One lattice kernel launch with its argument buffer; ``plan(ptrs, stream, omega)`` patches the leading pointer
    slots (the table's pointers: the pdf arrays, the neighbour mask, … and last the density / velocity arrays of an
    observed step, another slice every launch) and the relaxation rate, and launches on the plan's device
    (made current for the launch when it is not: the function handle belongs to that device's module)."""
    __slots__ = ('fn', 'nblocks', 'template', 'fmt', 'device', 'om_off', 'om_fmt', 'block')

    def __init__(self, fn, nblocks, template, nptr, device, om_off, om_code):
        self.fn, self.nblocks, self.template, self.fmt = fn, nblocks, template, f'<{nptr}Q'
        self.device, self.om_off, self.om_fmt = device, om_off, None if om_code is None else '<' + om_code
        self.block = 256

    def __call__(self, ptrs, stream, omega=None):
        from ..backends import hip_runtime as rt
        buf = bytearray(self.template)
        struct.pack_into(self.fmt, buf, 0, *ptrs)
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
