"""The force on a boundary object by momentum exchange: link lists, and the host side of the boundary-force kernels.

``boundary_links`` builds, from the flag array, the links ``(x, d)`` of one boundary object — ``x`` a fluid cell,
``x + c_d`` (periodic) a cell of the boundary — sorted by (direction, cell), and ``force_table`` the two doubles per
direction the kernels read: ``1 + α_d`` and ``β_d`` of the boundary's fused link ``f_in = α·f_d(x) + β``
(``boundaries.link_coefficients``), with ``(1 + α_d)·w_d`` added for zero-centred storage. ``WallForceKernels`` compiles
the text of ``_wall_force_source`` (hiprtc for gfx950, or gcc) and launches it:

    F = Σ_links c_d·((1 + α_d)·f_d(x) + β_d)                 ``force``   (gather-reduce, two launches, no atomics)
    g_d(x) += (1 + α_d)·Σ_a c_{d,a}·dF_a   on the links      ``adjoint`` (scatter, one thread per link)

The index type and the addressing of a launch are the lattice kernels' (``addressing_mode``: buffer resources
below 2 GiB, plain pointers from there on or with ``PSAD_LBM_ADDR=ptr``, 64-bit offsets from 2³¹ − 1 elements);
``PSAD_LBM_ADDR=ptr64`` forces the 64-bit pointer variant here (tests: the lattice kernels ignore that value).
"""
import ctypes
import os

import numpy as np

from . import _wall_force_source as WS
from ._lattice_kernels import _ptr, _reach, _stream, addressing_mode, lattice_strides
from .boundaries import link_form

__all__ = ['BoundaryLinks', 'WallForceKernels', 'boundary_links', 'force_table', 'DEFAULT_BLOCK_CAP']

# The most workgroups of ``lbm_wall_force``: one per CU of an MI355X (256). A workgroup more would wait for a CU, and
# every workgroup costs the second stage D more doubles to add in order; 256·256 links per pass cover the walls of a
# 192³ channel in six strided iterations.
DEFAULT_BLOCK_CAP = 256


def force_table(boundary, adjoint, lb_method, zero_centered=False):
    """``float64 [Q, 2]``: per direction ``(1 + α, β)`` of ``boundary``'s link, β with ``(1 + α)·w_d`` added for
    zero-centred storage (the kernels then read ``s = f − w``). Raises ``NotImplementedError`` naming the boundary
    when its links are not the fused affine form in one pdf: a link program or a neighbour link (``FixedDensity``,
    ``FreeSlip``, ``ZeroGradientOutflow``), or a density-weighted row (``βρ ≠ 0``) — there one link depends on every pdf
    of its cell, and several links of one cell would write the same gradient entries."""
    kind, form = link_form(boundary, adjoint, lb_method)
    if kind != 'affine':
        raise NotImplementedError(
            f'boundary force on {boundary.name} ({boundary!r}): its links are a {kind} link, not the fused form '
            'f_in = alpha*f_d(x) + beta in one pdf that the momentum-exchange kernels sum')
    if any(row[3] != 0.0 for row in form):
        raise NotImplementedError(
            f'boundary force on {boundary.name} ({boundary!r}): density-weighted links (beta_rho != 0) read every pdf '
            'of the cell, not one: the momentum-exchange kernels take links in one pdf')
    st = getattr(lb_method, 'stencil', lb_method)
    w = [float(v) for v in st.weights]
    tab = np.zeros((st.Q, 2), np.float64)
    for d, row in enumerate(form):
        if any(st.directions[d]):
            tab[d, 0] = 1.0 + row[0]
            tab[d, 1] = row[1] + (tab[d, 0] * w[d] if zero_centered else 0.0)
    return tab


def boundary_links(flags, stencil, flag_id):
    """``(cells, directions)`` of the links of the boundary with ``flag_id`` on ``flags`` (wall ids over the domain,
    0 = fluid): C-order cell indices (int32; int64 for lattices of 2³¹ − 1 cells and more) and direction indices
    (uint8), sorted by (direction, cell) — a wave reads one component, ascending cells."""
    f = np.asarray(flags)
    axes = tuple(range(f.ndim))
    fluid, wall = f == 0, f == flag_id
    cells, dirs = [], []
    for d, c in enumerate(stencil.directions):
        if not any(c):
            continue
        # wall[x + c_d] with periodic wrap (the kernels' neighbour mask has the same wrap)
        hit = np.flatnonzero((fluid & np.roll(wall, tuple(-int(v) for v in c), axis=axes)).ravel())
        cells.append(hit)
        dirs.append(np.full(hit.size, d, np.uint8))
    ctype = np.int32 if f.size < 2 ** 31 - 1 else np.int64
    return np.concatenate(cells).astype(ctype), np.concatenate(dirs)


class BoundaryLinks:
    """The link list of one boundary object on one flag array: ``cells``, ``directions`` (numpy) and ``table``
    (``force_table``); ``n`` links. ``operands`` are what a launch takes: the arrays in the kernels' index type, on
    the GPU target uploaded once per (device, index type)."""

    def __init__(self, boundary, cells, directions, table):
        self.boundary, self.cells, self.directions, self.table = boundary, cells, directions, table
        self.n = int(cells.size)
        self.max_cell = int(cells.max()) if self.n else -1
        self._host = {}
        self._dev = {}

    def operands(self, idx, device=None):
        """``(cells, directions, table)`` with cells of type ``idx`` ('int' / 'long long'): numpy arrays, or torch
        tensors on ``device``."""
        host = self._host.get(idx)
        if host is None:
            host = self._host[idx] = (np.ascontiguousarray(self.cells, np.int32 if idx == 'int' else np.int64),
                                      np.ascontiguousarray(self.directions, np.uint8),
                                      np.ascontiguousarray(self.table, np.float64).reshape(-1))
        if device is None:
            return host
        dev = self._dev.get((idx, device))
        if dev is None:
            import torch
            dev = self._dev[(idx, device)] = tuple(torch.from_numpy(a).to(device) for a in host)
        return dev


class WallForceKernels:
    """The boundary-force kernels of one (stencil, pdf dtype, target)."""

    def __init__(self, stencil, dtype, target):
        self.stencil, self.dtype, self.target = stencil, np.dtype(dtype), target
        if self.dtype not in (np.float16, np.float32, np.float64):
            raise NotImplementedError(f'boundary-force kernels for {self.dtype} pdfs')
        # the compute type: of the force and of its gradient
        self.cdtype = np.dtype(np.float64 if self.dtype == np.float64 else np.float32)
        self._fns = {}

    def source(self, idx='int', addr='buf'):
        return WS.emit(self.stencil, self.dtype.name, 'hip' if self.target == 'gpu' else 'c', idx, addr)

    def build(self):
        """Compile without a device: the three addressing variants (HIP), or the C library."""
        if self.target != 'gpu':
            return self._cpu_fn('lbm_wall_force')
        from ..backends import hip_runtime as rt
        return [rt.compile_hip(self.source(i, a), name='psad_lbm_wall_force.hip')
                for i, a in (('int', 'buf'), ('int', 'ptr'), ('long long', 'ptr'))]

    @staticmethod
    def mode(t):
        """``(idx, addr)`` of a launch on the pdf tensor ``t``: the lattice kernels' choice
        (``_lattice_kernels.addressing_mode``, a function of the tensor's reach alone); ``PSAD_LBM_ADDR=ptr64``:
        ('long long', 'ptr')."""
        if os.environ.get('PSAD_LBM_ADDR') == 'ptr64':
            return 'long long', 'ptr'
        return addressing_mode([t])

    @staticmethod
    def blocks(n, cap=None):
        """Workgroups of ``lbm_wall_force`` over ``n`` links: a function of ``n`` (and the cap) alone."""
        cap = DEFAULT_BLOCK_CAP if cap is None else int(cap)
        if cap < 1:
            raise ValueError(f'block cap {cap}: at least 1')
        return min(-(-int(n) // WS.BLOCK), cap)

    # -- checks ------------------------------------------------------------------------------------
    def _check(self, t, what):
        D, Q = self.stencil.D, self.stencil.Q
        if len(t.shape) != D + 1 or int(t.shape[D]) != Q:
            raise ValueError(f'{what} must be [*domain, {Q}], got {tuple(t.shape)}')
        if str(t.dtype).split('.')[-1] != self.dtype.name:
            raise TypeError(f'{what} must be {self.dtype.name}, got {t.dtype}')
        ncell = int(np.prod([int(v) for v in t.shape[:D]]))
        return ncell

    def _extent(self, t):
        shape = [int(v) for v in t.shape[:self.stencil.D]]
        return ([1] + shape)[-3:]

    # -- GPU ---------------------------------------------------------------------------------------
    def _gpu_fn(self, name, idx, addr, device):
        key = (name, idx, addr, device)
        fn = self._fns.get(key)
        if fn is None:
            from ..backends import hip_runtime as rt
            code = rt.compile_hip(self.source(idx, addr), name='psad_lbm_wall_force.hip')
            fn = self._fns[key] = rt.load_function(code, name, device)
        return fn

    def _launch(self, fn, nblocks, block, args, t, stream):
        import torch

        from ..backends import hip_runtime as rt
        st = _stream(stream, t)
        if t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device.index):
                rt.launch(fn, (nblocks,), (block,), args, st)
        else:
            rt.launch(fn, (nblocks,), (block,), args, st)

    def _array_args(self, t, idx):
        """The tail of both link kernels' arguments: n is put in front by the caller; Y, X, strides, bytes."""
        _, Y, X = self._extent(t)
        ik = 'i32' if idx == 'int' else 'i64'
        return [('i32', Y), ('i32', X)] + [(ik, s) for s in lattice_strides(t, self.stencil.D)] + \
            [('i64', _reach(t) * t.element_size())]

    def force(self, pdfs, links, out=None, cap=None, stream=None):
        """``F [D]`` (the compute type) of the state ``pdfs`` ``[*domain, q]`` (any strides) over ``links``; ``out``:
        written instead of a new array. ``cap``: the most workgroups of the first stage (``DEFAULT_BLOCK_CAP``)."""
        ncell = self._check(pdfs, 'pdfs')
        if links.max_cell >= ncell:
            raise ValueError('the link list does not belong to this lattice')
        D = self.stencil.D
        nb = self.blocks(links.n, cap)
        if self.target != 'gpu':
            F = np.zeros(D, self.cdtype) if out is None else out
            if links.n == 0:
                F[...] = 0
                return F
            if not (F.flags.c_contiguous and F.dtype == self.cdtype and F.shape == (D,)):
                raise ValueError('out must be a contiguous [D] array of the compute type')
            self._cpu('lbm_wall_force', pdfs, links, F)
            return F
        import torch

        from ..backends import hip_runtime as rt
        if not pdfs.is_cuda:
            raise ValueError('the HIP boundary-force kernels need a tensor on the GPU')
        cdt = getattr(torch, self.cdtype.name)
        F = torch.empty(D, dtype=cdt, device=pdfs.device) if out is None else out
        if F.dtype != cdt or tuple(F.shape) != (D,) or not F.is_contiguous() or F.device != pdfs.device:
            raise ValueError('out must be a contiguous [D] tensor of the compute type on the pdfs\' device')
        if links.n == 0:
            # (a grid of 0 is a launch error)
            F.zero_()
            return F
        idx, addr = self.mode(pdfs)
        cells, dirs, tab = links.operands(idx, pdfs.device)
        part = torch.empty(nb * D, dtype=torch.float64, device=pdfs.device)
        dev = pdfs.device.index
        args = rt.pack_args([('ptr', pdfs.data_ptr()), ('ptr', cells.data_ptr()), ('ptr', dirs.data_ptr()),
                             ('ptr', tab.data_ptr()), ('ptr', part.data_ptr()), ('i64', links.n)] +
                            self._array_args(pdfs, idx))
        self._launch(self._gpu_fn('lbm_wall_force', idx, addr, dev), nb, WS.BLOCK, args, pdfs, stream)
        args = rt.pack_args([('ptr', part.data_ptr()), ('ptr', F.data_ptr()), ('i32', nb)])
        self._launch(self._gpu_fn('lbm_wall_force_sum', idx, addr, dev), 1, WS.BLOCK, args, pdfs, stream)
        return F

    def adjoint(self, g, links, dF, stream=None):
        """``g_d(x) += (1 + α_d)·Σ_a c_{d,a}·dF_a`` on the links, in place (``g`` ``[*domain, q]``, any strides without
        overlap; ``dF`` ``[D]`` contiguous, the compute type)."""
        ncell = self._check(g, 'the adjoint array')
        if links.n == 0:
            return
        if links.max_cell >= ncell:
            raise ValueError('the link list does not belong to this lattice')
        D = self.stencil.D
        if tuple(dF.shape) != (D,) or str(dF.dtype).split('.')[-1] != self.cdtype.name:
            raise ValueError(f'dF must be [{D}] of {self.cdtype.name}, got {tuple(dF.shape)} {dF.dtype}')
        if self.target != 'gpu':
            return self._cpu('lbm_wall_force_adj', g, links, np.ascontiguousarray(dF))
        from ..backends import hip_runtime as rt
        if not g.is_cuda or dF.device != g.device or not dF.is_contiguous():
            raise ValueError('the adjoint array and dF must be on one GPU, dF contiguous')
        idx, addr = self.mode(g)
        cells, dirs, tab = links.operands(idx, g.device)
        args = rt.pack_args([('ptr', g.data_ptr()), ('ptr', cells.data_ptr()), ('ptr', dirs.data_ptr()),
                             ('ptr', tab.data_ptr()), ('ptr', dF.data_ptr()), ('i64', links.n)] +
                            self._array_args(g, idx))
        self._launch(self._gpu_fn('lbm_wall_force_adj', idx, addr, g.device.index), -(-links.n // WS.BLOCK),
                     WS.BLOCK, args, g, stream)

    # -- CPU ---------------------------------------------------------------------------------------
    def _cpu_fn(self, name):
        fn = self._fns.get(name)
        if fn is None:
            from ..backends.cpu_kernel import compile_c
            fn = self._fns[name] = compile_c(self.source(), name, openmp=False)
        return fn

    def _cpu(self, name, arr, links, vec):
        arr = np.asarray(arr)
        cells, dirs, tab = links.operands('long long')
        _, Y, X = self._extent(arr)
        ptrs = [_ptr(a) for a in (arr, cells, dirs, tab, vec)]
        P = (ctypes.c_void_p * len(ptrs))(*ptrs)
        N = (ctypes.c_longlong * 3)(links.n, Y, X)
        S = (ctypes.c_longlong * 4)(*lattice_strides(arr, self.stencil.D))
        B = (ctypes.c_longlong * 1)(0)
        Dv = (ctypes.c_double * 1)(0.0)
        self._cpu_fn(name)(P, N, S, B, Dv)
