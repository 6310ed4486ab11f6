"""Differentiable lattice Boltzmann time stepping (reference ``lbm/_autodiff_lbstep.py``).

``AutoDiffLatticeBoltzmannStep`` keeps the reference's constructor, field guessing and naming
(``_autodiff_lbstep.py:27-66,142-160``) but is not an lbmpy ``LatticeBoltzmannStep`` subclass (lbmpy is
absent): it owns its pdf arrays (the field's memory layout, lbmpy's default ``fzyx`` = one C-contiguous
plane per component) and runs the time loop the reference's ``run`` / ``run_backward`` drive through
lbmpy (``:336-398``) directly on the HIP kernels of an ``AutoDiffOp`` built with
``boundary_handling='periodic'``: the kernels wrap their reads (and the adjoint its writes) around the
lattice, so there are no ghost layers, no per-step ghost sync (lbmpy's ``_sync_src``) and no adjoint
fold-back — one kernel launch per step in each direction:

    forward step:  dst = stream-pull-collide(src)                      → swap
    adjoint step:  diffsrc = transposed kernel(diffdst, recorded src)  → swap
                   (scatter to x − c_i: for a fixed component i, x ↦ x − c_i is a bijection of the
                   periodic lattice, so every (component, cell) is written exactly once, no zero fill)

Deliberate deviations, each because the reference's behaviour is not a gradient:
* the adjoint is the ``DiffModes.TRANSPOSED`` form (``_autodiff.py:354-437``), not TF-MAD. TF-MAD
  evaluates ∂f/∂src at the unshifted cell (``_autodiff.py:102-109``), exact only for linear stencils, and
  its vector-field branch keeps only the last component's assignment (``_autodiff.py:138-152``); the
  collision is nonlinear and all components are needed.
* the backward of T steps needs each step's src state (the collision Jacobian depends on it): the forward
  records them (``record=True`` / the timestep op: T + 1 arrays, written in turn, no copies); the
  reference's ``run_backward`` re-uses whatever the arrays hold.

Rules made by ``create_lb_update_rule`` run on the lattice schedule (``_lattice_kernels``: one forward and one
adjoint kernel written for the lattice, any pdf strides, the op's internal states in the row-interleaved
``[z][y][q][x]`` layout) — which also carries no-slip walls (``set_boundary_including_adjoint``,
``_autodiff_lbstep.py:162-187``; half-way bounce-back fused into the pull, obstacle cells keep their state).
Other rules run on the ``AutoDiffOp`` kernels (periodic, no walls).
"""
import numpy as np
import sympy as sp

from .. import ps
from ..autodiff import AutoDiffOp
from ._lattice_kernels import LatticeKernels, fix_cells, neighbour_mask
from ._lattice_rule import lattice_rule
from ._lattice_source import CELL_FIELDS, density_links_message, link_rows
from ._method import LBStencil
from .boundaries import (AdjointBoundaryCondition, AdjointNoSlip, Boundary, BoundaryHandling, LBMethodView,  # noqa: F401
                         NoSlip, link_form)

__all__ = ['AutoDiffLatticeBoltzmannStep', 'PdfFieldNotDetectedException', 'SimulationResultsTensors']


class PdfFieldNotDetectedException(Exception):
    pass


class SimulationResultsTensors:
    """Same record as the reference (``_autodiff_lbstep.py:19-24``)."""

    def __init__(self, input_pdf_tensor, output_pdf_tensor, output_density_tensor, output_velocity_tensor):
        self.input_pdf_tensor = input_pdf_tensor
        self.output_pdf_tensor = output_pdf_tensor
        self.output_density_tensor = output_density_tensor
        self.output_velocity_tensor = output_velocity_tensor


def _lattice_sweeps(step, which, launches, fields=None, macro=None, before=None):
    """The lattice kernels over ``launches`` (tensor tuples of ``LatticeKernels.forward`` / ``adjoint``) on the
    current stream: one launch plan per distinct (shapes, strides) — the first, middle and last steps — and only
    the pointers packed per launch. ``fields``: the per-cell fields (``step._field_args``: kind → (array, adjoint)),
    bound to every launch; the adjoint launches add their share into each field's adjoint array. ``macro``: per launch
    None, or the density / velocity arrays of an observed step by name
    (``LatticeKernels.operands``) — those launches run the kernels' density / velocity variant, the others the plain
    kernels with no argument more. ``before``: per launch None, or a callable run (enqueued) before that launch — the
    boundary-force seeds, added into the adjoint array the launch reads."""
    K = step._lattice_kernels()
    mask = step._flag_arg()
    ids = step._ids_arg()
    cells = step._cells_arg()
    om = step._omega_of()
    macro = macro or [None] * len(launches)
    before = before or [None] * len(launches)
    if not step._gpu:
        # the C kernels on numpy arrays (both adjoint passes in one call)
        for ts, m, pre in zip(launches, macro, before):
            if pre is not None:
                pre()
            K.run(which, list(ts), om, mask, ids, fields, m)
        return
    stream = _torch()._C._cuda_getCurrentRawStream(launches[0][0].device.index)
    rho = K.rho_buffer(launches[0][0]) if which == 'adj' and K.link_pass else None
    # once: the launches differ in their pdf arrays (the leading pointer slots) and, the observed ones, in the
    # density / velocity arrays (the trailing ones)
    mptr = K.pointers(which, K.operands((), mask, ids, fields, rho))[len(launches[0]):]
    mnames = K.table_pointer_names(which, True)[len(launches[0]) + len(mptr):]
    plans = {}
    for ts, m, pre in zip(launches, macro, before):
        if pre is not None:
            pre()
        sig = tuple(t.stride() for t in ts) + (m is not None,)
        plan = plans.get(sig)
        if plan is None:
            plan = plans[sig] = K.plan(which, list(ts), mask, om, ids, fields, macro=m)
        plan(tuple(t.data_ptr() for t in ts) + mptr +
             (tuple(0 if m.get(n) is None else m[n].data_ptr() for n in mnames) if m else ()), stream, om)
        # link-program walls (HIP): the fix-up kernels over the cells next to them
        K.fix_launch(which, list(ts), mask, om, ids, fields, cells, stream, m)
        if rho is not None:
            # the second pass of density-weighted walls (and, on the CPU, link programs) on this launch's output
            K.rho_pass(ts[2], mask, rho, stream)


def _guess_src_dst_field_from_update_rule(update_rule, src_hint, dst_hint):
    """``_autodiff_lbstep.py:27-46``: a string hint means "find the one ≥9-component field"."""
    src_candidates = dst_candidates = None
    if isinstance(src_hint, str):
        src_candidates = [f for f in update_rule.free_fields if f.index_dimensions == 1 and f.index_shape[0] >= 9]
        if len(src_candidates) != 1:
            raise PdfFieldNotDetectedException(
                'Could not guess source PDF field from update rule.' +
                'Please specify the field explicitly in the constructor of AutoDiffLatticeBoltzmannStep!')
    if isinstance(dst_hint, str):
        dst_candidates = [f for f in update_rule.bound_fields if f.index_dimensions == 1 and f.index_shape[0] >= 9]
        if len(dst_candidates) != 1:
            raise PdfFieldNotDetectedException(
                'Could not guess temporary PDF field from update rule.' +
                'Please specify the field explicitly in the constructor of AutoDiffLatticeBoltzmannStep!')
    src = src_hint if isinstance(src_hint, ps.Field) else src_candidates[0]
    dst = dst_hint if isinstance(dst_hint, ps.Field) else dst_candidates[0]
    return src, dst


def _torch():
    import torch
    return torch


class AutoDiffLatticeBoltzmannStep:
    """Forward and adjoint lattice Boltzmann time steps on one periodic domain.

    ``update_rule``: a stream-pull-collide ``AssignmentCollection`` (``lbm.create_lb_update_rule``), its pdf
    fields found as in the reference. ``domain_size``: the spatial extent (without ghost layers).
    ``relaxation_rate`` sets the value of the rule's free scalar (``omega``) unless given as
    ``kernel_params``; a rule whose rate is read from a field (``relaxation_rate=w.center``, a per-cell ω) has no such
    scalar: the field is an additional input of the step, ``create_timestep_op(T).apply(pdfs, *extras)`` in name order,
    and the backward returns its adjoint summed over the steps (a trainable scalar rate: pass ``w0.expand(*domain)``).
    A rule with a per-cell solid fraction (``solid_fraction=s.center``, partial bounce-back) takes the σ field the same
    way and returns ``dσ``.
    ``target``: ``'gpu'`` (HIP kernels on torch tensors) or ``'cpu'`` (the C kernels on
    numpy arrays)."""

    def __init__(self, update_rule, src_pdf_field='', tmp_pdf_field='', time_constant_fields=(), *args,
                 constant_fields=(), domain_size=None, relaxation_rate=None, target='gpu', kernel_params=None,
                 device=None, **method_parameters):
        if args:
            raise TypeError('positional lbmpy LatticeBoltzmannStep arguments are not supported: pass keywords')
        src, tmp = _guess_src_dst_field_from_update_rule(update_rule, src_pdf_field, tmp_pdf_field)
        self.pdf_field = src
        self.temporary_field = tmp
        self._pdf_arr_name = src.name
        self._tmp_arr_name = tmp.name
        self._target = str(target).lower()
        if self._target not in ('gpu', 'cpu'):
            raise ValueError("target must be 'gpu' or 'cpu'")
        self._gpu = self._target == 'gpu'
        self._update_rule = update_rule
        self.method = getattr(update_rule, 'stencil', None) or LBStencil(
            {(2, 9): 'D2Q9', (3, 19): 'D3Q19', (3, 27): 'D3Q27'}[(src.spatial_dimensions, int(src.index_shape[0]))])
        if domain_size is None:
            if not src.has_fixed_shape:
                raise ValueError('domain_size is required for variable-size pdf fields')
            domain_size = tuple(int(s) for s in src.spatial_shape)
        self.domain_size = tuple(int(s) for s in domain_size)
        if len(self.domain_size) != src.spatial_dimensions or min(self.domain_size) < 2:
            raise ValueError(f'domain_size {self.domain_size} does not fit the {src.spatial_dimensions}-D pdf field')
        # periodic kernels (wrapped reads, every cell written) and the transposed adjoint — for the rules of
        # ``create_lb_update_rule`` written through the collision's structure (``create_lb_adjoint_rule``)
        backward = None
        # the op's forward input fields (the fields the rule reads, sorted by name — transposed_backward's order)
        read = {a.field for asg in update_rule.all_assignments for a in sp.sympify(asg.rhs).atoms(ps.Field.Access)}
        self._additional_fields = [f for f in sorted(read, key=str) if f not in (src, tmp)]
        rr = getattr(update_rule, 'relaxation_rate', None)
        rate_fields = sorted({a.field for a in sp.sympify(rr).atoms(ps.Field.Access)}, key=str) if rr is not None else []
        for w in rate_fields:
            if w.index_dimensions:
                raise ValueError(f"relaxation-rate field '{w.name}' has an index dimension: a per-cell relaxation rate "
                                 'is a scalar field (one value per cell)')
        # (a force term that depends on the pdfs — Guo's, through u — is not in that structure: the generic
        # transposed derivation then; the 'simple' term is a constant and changes no derivative. Nor is a rate read
        # from a field — any additional input field: the structured rule has the pdf adjoint only)
        from ._method import force_is_field
        if getattr(update_rule, 'stencil', None) is not None and not time_constant_fields and \
                getattr(update_rule, 'force_model', None) in (None, 'simple') and \
                not force_is_field(getattr(update_rule, 'force', None)) and not self._additional_fields and \
                getattr(update_rule, 'smagorinsky', None) is None and \
                getattr(update_rule, 'solid_fraction', None) is None:
            # (nor is the Smagorinsky model's rate, a function of the pdfs: the generic derivation as well; nor the
            # partial bounce-back blend of a solid fraction, whatever σ is)
            from ._method import create_lb_adjoint_rule
            backward = create_lb_adjoint_rule(update_rule)
        # the rule's AutoDiffOp (its kernels are the schedule for rules the lattice kernels do not take, and its
        # transposed derivation — tens of seconds of sympy for a D3Q19 force-field rule — is only needed then):
        # built on first use
        self._autodiff_op = None
        self._autodiff_args = dict(forward_assignments=update_rule, op_name='LBM', boundary_handling='periodic',
                                   diff_mode='transposed', time_constant_fields=list(time_constant_fields) or None,
                                   constant_fields=list(constant_fields), backward_assignments=backward)
        self._diff_prefix = 'diff'
        scalars = sorted({s for a in update_rule.all_assignments for s in a.rhs.free_symbols
                          if isinstance(s, sp.Symbol) and not isinstance(s, ps.Field.Access)}
                         - {a.lhs for a in update_rule.subexpressions}, key=str)
        self.kernel_params = dict(kernel_params or {})
        for s in scalars:
            if s.name not in self.kernel_params:
                if relaxation_rate is None:
                    raise ValueError(f"scalar '{s.name}' of the update rule needs a value (relaxation_rate / "
                                     f"kernel_params)")
                self.kernel_params[s.name] = float(relaxation_rate)
        self._device = device
        self._arrays = {}
        self._records = None
        # the lattice schedule for the rules of create_lb_update_rule (``lattice_rule``: which rules, and what their
        # kernels are built from); walls need it. ``_lattice``: the step's LatticeKernels by wall set, None for a rule
        # that runs on the AutoDiffOp kernels
        self._lattice_rule = rule = lattice_rule(update_rule, src, time_constant_fields)
        self._lattice = None if rule is None else {}
        # the per-cell fields the lattice kernels take as arrays, by kind (``CELL_FIELDS``) and by name
        self._cell_fields = {f.kind: None if rule is None else rule.fields[f.kind] for f in CELL_FIELDS}
        self._force_field, self._omega_field, self._solid_field = (self._cell_fields[k] for k in
                                                                   ('force', 'omega', 'solid'))
        self._lattice_mrt = None if rule is None else rule.mrt
        # the kernels' scalar ω argument (unused with an ω field)
        how, value = (None, None) if rule is None else rule.rate
        self._omega_of = {None: None, 'field': lambda: 0.0, 'param': lambda: float(self.kernel_params[value]),
                          'number': lambda: float(value)}[how]
        self._boundary = BoundaryHandling(self.domain_size, on_change=self._flags_changed)
        # the lb_method the boundaries see: the stencil plus the rule's compressibility (FixedDensity reads it)
        self._bc_method = LBMethodView(self.method, getattr(update_rule, 'compressible', False))
        self._adjoint_boundary_conditions = {}
        self._flag_dev = None
        self._ids_dev = None

    @property
    def _autodiff(self):
        if self._autodiff_op is None:
            self._autodiff_op = AutoDiffOp(**self._autodiff_args)
            fwd = getattr(self, '_forward_only', None)
            if fwd is not None:
                # the forward kernel that already ran (``_forward_kernel``) IS the op's: one compiled kernel, whose
                # ``last_variant`` reports the launches made before the op existed
                self._autodiff_op._kernels[('forward', fwd.target)] = fwd
        return self._autodiff_op

    def _adjoint_name(self, field):
        """The adjoint array name of an additional input field (the op's field map once it exists; the AdjointField
        naming ``diff<name>`` before, which is what that map holds)."""
        if self._autodiff_op is not None:
            return self._autodiff_op.adjoint_name(field)
        return self._diff_prefix + field.name

    # -- reference-named properties ----------------------------------------------------------------
    @property
    def backward_pdf_array_name(self):
        return "diff" + self._tmp_arr_name

    @property
    def _backward_tmp_array_name(self):
        return "diff" + self._pdf_arr_name

    @property
    def forward_assignments(self):
        return self._autodiff.forward_assignments

    @property
    def backward_assignments(self):
        return self._autodiff.backward_assignments

    @property
    def lb_method(self):
        return self.method

    @property
    def autodiff_op(self):
        return self._autodiff

    # -- arrays ------------------------------------------------------------------------------------
    def _alloc(self, zero=True):
        """A pdf array in the field's memory layout, spatial axes first in the returned view (``zero=False``:
        uninitialised, for arrays a kernel writes completely)."""
        Q = int(self.pdf_field.index_shape[0])
        dims = list(self.domain_size)
        dt = self.pdf_field.dtype.numpy_dtype
        if self._gpu:
            torch = _torch()
            tdt = getattr(torch, np.dtype(dt).name)
            dev = self._device or torch.device('cuda', torch.cuda.current_device())
            new = torch.zeros if zero else torch.empty
            if self.pdf_field.is_soa:
                return new([Q] + dims, dtype=tdt, device=dev).permute(*range(1, len(dims) + 1), 0)
            return new(dims + [Q], dtype=tdt, device=dev)
        new = np.zeros if zero else np.empty
        if self.pdf_field.is_soa:
            return np.moveaxis(new([Q] + dims, dtype=dt), 0, -1)
        return new(dims + [Q], dtype=dt)

    def empty_pdfs(self):
        """An uninitialised pdf tensor in the step's memory layout (``[*domain_size, q]`` view; for ``fzyx``
        one contiguous plane per component) — inputs in this layout enter the timestep op without a copy."""
        return self._alloc(zero=False)

    def _as_layout(self, t):
        """``t`` itself if it has the step's memory layout, else a copy in it."""
        ref = self._array(self._pdf_arr_name)
        if tuple(t.shape) == tuple(ref.shape) and tuple(t.stride()) == tuple(ref.stride()) and t.dtype == ref.dtype:
            return t
        out = self._alloc(zero=False)
        out.copy_(t)
        return out

    def _internal_states(self, n):
        """``n`` states only the time-step op sees, in the row-interleaved layout (lattice schedule), as views
        of one allocation."""
        if n <= 0:
            return []
        torch = _torch()
        dev = self._device or torch.device('cuda', torch.cuda.current_device())
        Q = int(self.pdf_field.index_shape[0])
        dims = list(self.domain_size)
        base = torch.empty([n] + dims[:-1] + [Q, dims[-1]],
                           dtype=getattr(torch, np.dtype(self.pdf_field.dtype.numpy_dtype).name), device=dev)
        return list(base.transpose(-1, -2).unbind(0))

    def _lattice_input_ok(self, t):
        """A tensor the lattice kernels take as it is: ``[*domain, q]`` of the pdf dtype on the step's device."""
        ref = self._array(self._pdf_arr_name)
        return tuple(t.shape) == tuple(ref.shape) and t.dtype == ref.dtype and t.device == ref.device

    def _array(self, name):
        if name not in self._arrays:
            self._arrays[name] = self._alloc()
        return self._arrays[name]

    @property
    def pdf_array(self):
        """The current pdfs (``[*domain_size, q]``)."""
        return self._array(self._pdf_arr_name)

    def set_pdfs(self, pdfs):
        self._array(self._pdf_arr_name)[...] = pdfs
        self._records = None

    # -- boundaries (``_autodiff_lbstep.py:162-187``) --------------------------------------------------
    @property
    def boundary_handling(self):
        """The obstacle flags (``BoundaryHandling.set_boundary``); forward and adjoint read the same flags."""
        return self._boundary

    @property
    def backward_boundary_handling(self):
        return self._boundary

    def set_boundary_including_adjoint(self, boundary_condition, slice_obj=None, mask_callback=None, mask_array=None,
                                       adjoint_boundary_condition=None):
        """Set ``boundary_condition`` (a ``Boundary``: ``NoSlip``, ``UBB``, ``FixedDensity``, any boundary whose
        link reads only the fluid cell's own pdfs, or a ``NeighbourBoundary`` — ``FreeSlip``, ``ZeroGradientOutflow`` —
        whose link reads neighbouring fluid cells, ``boundaries.link_form``) on the selected cells for the forward
        AND the adjoint steps (the reference's signature; the adjoint condition defaults to
        ``AdjointBoundaryCondition(bc)``, derived from the forward link by AD)."""
        if not isinstance(boundary_condition, Boundary) or \
                isinstance(boundary_condition, (AdjointNoSlip, AdjointBoundaryCondition)):
            raise NotImplementedError(f'boundary {boundary_condition!r}: needs a forward Boundary object')
        if self._lattice is None:
            raise NotImplementedError('walls need the lattice schedule (a create_lb_update_rule rule without '
                                      'time-constant or additional fields)')
        if adjoint_boundary_condition is None:
            adjoint_boundary_condition = self._adjoint_boundary_conditions.setdefault(
                boundary_condition, AdjointBoundaryCondition(
                    boundary_condition, time_constant_fields=list(self._autodiff_args['time_constant_fields'] or []),
                    constant_fields=list(self._autodiff_args['constant_fields'] or []) + ['indexVector']))
        elif not isinstance(adjoint_boundary_condition, (AdjointNoSlip, AdjointBoundaryCondition)):
            raise NotImplementedError(f'adjoint boundary {adjoint_boundary_condition!r}')
        kind, form = link_form(boundary_condition, adjoint_boundary_condition, self._bc_method)   # or raise
        # links that read a density (density-weighted, link programs, neighbour links) are built for plain float32 /
        # float64 pdfs only (``LatticeSource``)
        reads_density = any(p is not None for p in form) if kind != 'affine' else \
            any(t.reads_density for t in link_rows([form])[0])
        if reads_density:
            for on, what in ((getattr(self._update_rule, 'zero_centered', False), 'zero_centered pdfs'),
                             (np.dtype(self.pdf_field.dtype.numpy_dtype) == np.float16, 'float16 pdfs')):
                if on:
                    raise NotImplementedError(density_links_message(what, f'boundary {boundary_condition!r}'))
        self._boundary.set_boundary(boundary_condition, slice_obj, mask_callback=mask_callback, mask_array=mask_array,
                                    adjoint=adjoint_boundary_condition)

    def _flags_changed(self):
        self._flag_dev = None
        self._ids_dev = None
        self._links_cached = None
        self._force_links = {}
        self._force_tables = {}
        self._records = None

    # -- boundary force (momentum exchange) --------------------------------------------------------
    def boundary_links(self, boundary):
        """The links of ``boundary`` (a boundary object set on this step) as a ``BoundaryLinks``: ``cells`` — the fluid
        cells ``x`` with ``x + c_d`` (periodic) a cell of the boundary, as C-order cell indices —, their
        ``directions`` ``d``, sorted by (direction, cell), and ``table`` ``[Q, 2]``: ``(1 + α_d, β_d)`` of the boundary's
        link (``_wall_force.force_table``). Built with numpy from the flags, once per flag change (and uploaded once on
        the GPU target). ``ValueError``: a boundary never set on the step; ``NotImplementedError``: a boundary whose
        links are not the fused form in one pdf."""
        from ._wall_force import BoundaryLinks, boundary_links
        if not isinstance(boundary, Boundary) or boundary not in self._boundary.conditions:
            raise ValueError(f'boundary {boundary!r} was never set on this step (set_boundary_including_adjoint)')
        table = self._force_table(boundary)
        cache = self.__dict__.setdefault('_force_links', {})
        links = cache.get(boundary)
        if links is None:
            cells, dirs = boundary_links(self._boundary.flags, self.method, self._boundary.conditions[boundary])
            links = cache[boundary] = BoundaryLinks(boundary, cells, dirs, table)
        return links

    def _force_table(self, boundary):
        """``force_table`` of a boundary set on the step, memoised until the next ``set_boundary`` (a boundary object is
        not to be changed once set: set it again after changing, say, a ``UBB``'s velocity)."""
        from ._wall_force import force_table
        tabs = self.__dict__.setdefault('_force_tables', {})
        if boundary not in tabs:
            tabs[boundary] = force_table(boundary, self._boundary.adjoints[self._boundary.conditions[boundary]],
                                         self._bc_method, getattr(self._update_rule, 'zero_centered', False))
        return tabs[boundary]

    def _wall_force_kernels(self):
        from ._wall_force import WallForceKernels
        k = self.__dict__.get('_wall_force')
        if k is None:
            k = self._wall_force = WallForceKernels(self.method, self.pdf_field.dtype.numpy_dtype, self._target)
        return k

    def _force_spec(self, spec):
        """``boundary_force_outputs`` as a list of ``(boundary, k)``: a boundary, a ``(boundary, k)`` pair or a list
        of those, ``k ≥ 1`` (default 1); every boundary checked (``boundary_links``)."""
        if isinstance(spec, Boundary) or (isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], Boundary)
                                          and not isinstance(spec[1], Boundary)):
            spec = [spec]
        out = []
        for e in spec:
            b, k = (e, 1) if isinstance(e, Boundary) else e
            if isinstance(k, (float, bool)) or int(k) < 1:
                raise ValueError(f'boundary_force_outputs: (boundary, k) with an int k >= 1, got k = {k!r}')
            self.boundary_links(b)
            out.append((b, int(k)))
        return out

    def create_boundary_force_op(self, boundary, backend='torch_native', block_cap=None):
        """A ``torch.autograd.Function`` for the force the fluid exerts on ``boundary`` by momentum exchange
        (lbmpy's ``force_on_boundary``): ``Op.apply(pdfs)`` with a state ``pdfs`` ``[*domain, q]`` of the step's dtype
        (post-collision pdfs — what the time-step op takes and returns; any strides) returns ``force [D]`` in the
        compute type (float32 for float16 / float32 pdfs, float64 for float64):

            F = Σ_links c_d·((1 + α_d)·f_d(x) + β_d)       over the links (x, d) of ``boundary`` (``boundary_links``)

        Its backward returns a zeroed array of ``pdfs``' shape plus ``(1 + α_d)·c_d·dF`` on the links. The link list
        is taken at every apply (``set_boundary`` between two applies changes it). ``block_cap``: the most workgroups
        of the HIP reduction's first stage (``_wall_force.DEFAULT_BLOCK_CAP``)."""
        if str(backend).lower() not in ('torch_native', 'torch'):
            raise NotImplementedError(f"backend '{backend}': only the torch backends are built")
        self.boundary_links(boundary)               # the refusals, at creation
        torch = _torch()
        step, gpu = self, self._gpu
        K = self._wall_force_kernels()
        pdt = np.dtype(self.pdf_field.dtype.numpy_dtype)
        cdt = getattr(torch, K.cdtype.name)

        class LbmBoundaryForce(torch.autograd.Function):
            @staticmethod
            def forward(ctx, pdfs):
                links = step.boundary_links(boundary)
                if tuple(pdfs.shape) != tuple(step.domain_size) + (step.method.Q,) or \
                        pdfs.dtype != getattr(torch, pdt.name):
                    raise TypeError(f'{LbmBoundaryForce.__name__}.apply(pdfs): pdfs [*{step.domain_size}, '
                                    f'{step.method.Q}] of {pdt.name}, got {tuple(pdfs.shape)} {pdfs.dtype}')
                ctx.links = links
                x = pdfs.detach()
                # (the gradient's layout: the input's, kept as a tensor without memory)
                ctx.like = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device='meta')
                if gpu:
                    return K.force(x, links, cap=block_cap)
                return torch.from_numpy(K.force(x.cpu().numpy(), links))

            @staticmethod
            def backward(ctx, dF):
                links, like = ctx.links, ctx.like           # (small, kept: a retained graph runs this again)
                g = torch.zeros_like(like, device=dF.device if gpu else 'cpu')
                d = dF.detach().to(cdt).contiguous()
                if gpu:
                    K.adjoint(g, links, d)
                else:
                    K.adjoint(g.numpy(), links, d.cpu().numpy())
                return g

        LbmBoundaryForce.lb_step = self
        LbmBoundaryForce.boundary = boundary
        return LbmBoundaryForce

    def _flag_arg(self):
        """The cells' neighbour masks for the wall kernels (computed once per flag change), None without walls."""
        if not self._boundary.has_walls:
            return None
        if self._flag_dev is None:
            if self._gpu:
                torch = _torch()
                dev = self._device or torch.device('cuda', torch.cuda.current_device())
                fix = self._fix_mask()
                self._flag_dev = neighbour_mask(torch.from_numpy(self._boundary.flags.copy()).to(dev), self.method,
                                                torch, fix=fix)
                self._cells_dev = None if fix is None else \
                    torch.from_numpy(np.flatnonzero(fix.ravel()).astype(np.int32)).to(dev)
            else:
                self._flag_dev = neighbour_mask(self._boundary.flags, self.method, np)
        return self._flag_dev

    def _fix_mask(self):
        """The fluid cells next to link-program walls, and the fluid cells that neighbour links of those read
        (``FIX_BIT``: the HIP fix-up kernels' list), None if no boundary is a link program."""
        progs = self._programs()
        if progs is None:
            return None
        return fix_cells(self._boundary.flags, self.method, [k for k, p in enumerate(progs) if p is not None], progs)

    def _cells_arg(self):
        """The fix-up kernels' cell list (int32 on the device), None without link programs (or on the CPU)."""
        if not self._gpu or self._flag_arg() is None:
            return None
        return getattr(self, '_cells_dev', None)

    def _links(self):
        """The wall kernels' link tables (None: every wall a plain bounce-back, or no walls), derived once per
        boundary change (``link_form`` differentiates each boundary's sympy link: not per step)."""
        return self._link_data()[0]

    def _programs(self):
        """The link programs of the walls the fused form does not take (None if there are none)."""
        return self._link_data()[1]

    def _link_data(self):
        cached = getattr(self, '_links_cached', None)
        if cached is None:
            cached = self._links_cached = (self._boundary.link_tables(self._bc_method) if self._boundary.has_walls
                                           else (None, None))
        return cached

    def _ids_arg(self):
        """The cells' wall ids for kernels with link tables (the flag array on the kernels' device), else None."""
        if self._links() is None:
            return None
        if getattr(self, '_ids_dev', None) is None:
            if self._gpu:
                torch = _torch()
                dev = self._device or torch.device('cuda', torch.cuda.current_device())
                self._ids_dev = torch.from_numpy(self._boundary.flags.copy()).to(dev)
            else:
                self._ids_dev = np.ascontiguousarray(self._boundary.flags)
        return self._ids_dev

    def _lattice_kernels(self):
        walls = self._boundary.has_walls
        links, programs = self._link_data()
        key = (walls, links, programs)
        k = self._lattice.get(key)
        if k is None:
            rule = self._lattice_rule
            k = self._lattice[key] = LatticeKernels(
                self.method, getattr(self._update_rule, 'compressible', False), self.pdf_field.dtype.numpy_dtype,
                walls, self._target, links, rule.force_model, rule.force, force_field=self._force_field is not None,
                trt=rule.trt, programs=programs, mrt=rule.mrt, omega_field=self._omega_field is not None,
                zero_centered=getattr(self._update_rule, 'zero_centered', False), smagorinsky=rule.smagorinsky,
                solid_field=self._solid_field is not None)
        return k

    # -- kernels -----------------------------------------------------------------------------------
    def _kernels(self):
        op = self._autodiff
        if self._gpu:
            return op.forward_ast_gpu.compile(), op.backward_ast_gpu.compile()
        return op.forward_ast_cpu.compile(), op.backward_ast_cpu.compile()

    def _fwd(self, src, dst, extra):
        if self._lattice is not None:
            return self._lattice_kernels().run('fwd', [src, dst], self._omega_of(), self._flag_arg(), self._ids_arg(),
                                               self._field_args(extra), cells=self._cells_arg())
        kf = self._forward_kernel()
        kf(**{self._pdf_arr_name: src, self._tmp_arr_name: dst}, **extra, **self.kernel_params)

    def _forward_kernel(self):
        """The rule's forward kernel on the AutoDiffOp schedule. While the op does not exist yet — its transposed
        derivation takes tens of seconds for a rule with square roots or a force field — a forward run compiles the
        rule alone: the same assignments, boundary handling and kernel name as the op's forward kernel."""
        if self._autodiff_op is not None:
            return self._kernels()[0]
        if getattr(self, '_forward_only', None) is None:
            from ..autodiff import AutoDiffBoundaryHandling
            from ..backends.kernel_ir import StencilKernel
            tgt = 'gpu' if self._gpu else 'cpu'
            self._forward_only = StencilKernel(self._update_rule,
                                               boundary_handling=AutoDiffBoundaryHandling('periodic'),
                                               function_name=f'LBM_forward_{tgt}', target=tgt)
        return self._forward_only.compile()

    def _field_args(self, extra, adjoints=None):
        """The per-cell fields of a lattice launch (``LatticeKernels.run``): kind → (the field's array from ``extra``,
        by the field's name; its adjoint array from ``adjoints``, by kind, or None) for the fields the rule reads."""
        fields = {}
        for row in CELL_FIELDS:
            f = self._cell_fields[row.kind]
            if f is None:
                continue
            try:
                fields[row.kind] = (extra[f.name], (adjoints or {}).get(row.kind))
            except (KeyError, TypeError):
                raise ValueError(f"the update rule reads the {row.what} '{f.name}': pass its array "
                                 "(extra={name: array})") from None
        return fields

    def _field_adjoints(self, extra_adj):
        """Kind → the adjoint array (accumulated into) of every per-cell field the rule reads, from ``extra_adj`` by
        the field's adjoint name."""
        adjoints = {}
        for row in CELL_FIELDS:
            if self._cell_fields[row.kind] is not None:
                name = self._adjoint_name(self._cell_fields[row.kind])
                if name not in (extra_adj or {}):
                    raise ValueError(f"the {row.what}'s adjoint '{name}' needs an array (extra_adj), accumulated into")
                adjoints[row.kind] = extra_adj[name]
        return adjoints

    def _zeroed_field_adjoints(self, ex, extras, zeros_like):
        """For the adjoint sweep of a time-step op: ``(dex, fields)`` — by name a zeroed array like each additional
        input of ``ex`` (every step's adjoint launch adds its share into it) and the sweep's per-cell fields with
        those arrays as their adjoints."""
        dex = {f.name: zeros_like(ex[f.name]) for f in extras}
        return dex, self._field_args(ex, {k: dex[f.name] for k, f in self._cell_fields.items() if f is not None})

    def _adjoint_launches(self, records, g, ping, out):
        """The T adjoint launches ``(state t, adjoint of state t + 1, adjoint of state t)``, t = T − 1 … 0: the adjoints
        of states T − 1 … 1 alternate between the arrays ``ping``; the gradient (the adjoint of state 0) is ``out``."""
        T = len(records)
        cur, launches = g, []
        for t in reversed(range(T)):
            nxt = out if t == 0 else ping[(T - 1 - t) % 2]
            launches.append((records[t], cur, nxt))
            cur = nxt
        return launches

    def _bwd(self, src, diffdst, diffsrc, extra, extra_adj):
        if self._lattice is not None:
            fields = self._field_args(extra, self._field_adjoints(extra_adj))
            return self._lattice_kernels().run('adj', [src, diffdst, diffsrc], self._omega_of(), self._flag_arg(),
                                               self._ids_arg(), fields, cells=self._cells_arg())
        _, kb = self._kernels()
        kb(**{self._pdf_arr_name: src, 'diff' + self._tmp_arr_name: diffdst, 'diff' + self._pdf_arr_name: diffsrc},
           **extra, **extra_adj, **self.kernel_params)

    # -- time loops --------------------------------------------------------------------------------
    def time_step(self, extra=None):
        """One forward step on the owned arrays: stream-pull-collide, swap. While recording, the step writes
        into a fresh array and its src stays as the record (no copies)."""
        a = self._array(self._pdf_arr_name)
        if self._records is not None:
            self._records.append(a)
            b = self._alloc(zero=False)
            self._fwd(a, b, extra or {})
            self._arrays[self._pdf_arr_name] = b
            return
        b = self._array(self._tmp_arr_name)
        self._fwd(a, b, extra or {})
        self._arrays[self._pdf_arr_name], self._arrays[self._tmp_arr_name] = b, a

    def run(self, time_steps, record=False, extra=None):
        """``time_steps`` forward steps; ``record=True`` keeps each step's src state for ``run_backward``
        (T + 1 pdf arrays live until the backward has consumed them)."""
        self._records = [] if record else None
        for _ in range(int(time_steps)):
            self.time_step(extra)

    def backward_time_step(self, src_state, extra=None, extra_adj=None):
        """One adjoint step: diffsrc = Kᵀ(diffdst) with the collision Jacobian at ``src_state``."""
        g_dst = self._array(self.backward_pdf_array_name)
        g_src = self._array(self._backward_tmp_array_name)
        self._bwd(src_state, g_dst, g_src, extra or {}, extra_adj or {})
        self._arrays[self.backward_pdf_array_name], self._arrays[self._backward_tmp_array_name] = g_src, g_dst

    def set_adjoint_pdfs(self, grad):
        """The adjoint of the current (final) pdfs."""
        self._array(self.backward_pdf_array_name)[...] = grad

    @property
    def adjoint_pdf_array(self):
        return self._array(self.backward_pdf_array_name)

    def run_backward(self, time_steps, extra=None, extra_adj=None):
        """``time_steps`` adjoint steps in reverse over the states the last ``run(..., record=True)`` kept;
        the result is ``adjoint_pdf_array`` (gradient w.r.t. the pdfs before that run)."""
        if self._records is None or len(self._records) < int(time_steps):
            raise RuntimeError('run_backward needs the states of a preceding run(time_steps, record=True)')
        for t in range(int(time_steps)):
            self.backward_time_step(self._records[-1 - t], extra, extra_adj)
        self._records = self._records[:len(self._records) - int(time_steps)]

    # -- torch ops ---------------------------------------------------------------------------------
    def create_timestep_op(self, num_time_steps, input_field_to_tensor_dict=None, backend='torch_native',
                           macroscopic_outputs=None, boundary_force_outputs=None):
        """A ``torch.autograd.Function`` for ``num_time_steps`` steps: ``Op.apply(pdfs)`` with the interior
        pdfs (``[*domain_size, q]``) returns the pdfs after the steps; its backward runs the adjoint steps
        in reverse over the recorded states (``_autodiff_lbstep.py:189-247``; the reference's
        ``torch_native`` backend ignores the loops and differentiates one kernel launch).

        ``macroscopic_outputs``: ``True`` or an int ``k ≥ 1`` — the op returns ``(pdfs, rho, vel)`` with the density
        ``rho [n, *domain]`` and the velocity ``vel [n, *domain, D]`` of the states k, 2k, …, nk, ``n = T // k``
        (state t: the output of step t), written by the lattice kernels that compute those states, and its backward
        takes their gradients too (``_observed_timestep_op``).

        ``boundary_force_outputs``: a boundary object set on the step, a ``(boundary, k)`` pair (``k ≥ 1``, default 1)
        or a list of those — the op returns its usual outputs followed by one ``force [n, D]`` per entry: the
        momentum-exchange force on that boundary (``create_boundary_force_op``) of the states k, 2k, …, nk,
        ``n = T // k``, computed on the recorded states in place; its backward takes their gradients too."""
        if str(backend).lower() not in ('torch_native', 'torch'):
            raise NotImplementedError(f"backend '{backend}': only the torch backends are built")
        extras = list(self._additional_fields)
        known = {self.pdf_field.name} | {f.name for f in extras}
        unknown = [getattr(f, 'name', f) for f in (input_field_to_tensor_dict or {}) if getattr(f, 'name', f) not in known]
        if unknown:
            raise ValueError(f'input fields {unknown} are not read by the update rule (inputs: {sorted(known)})')
        if macroscopic_outputs is False:
            macroscopic_outputs = None
        if boundary_force_outputs is not None:
            return self._observed_timestep_op(int(num_time_steps), macroscopic_outputs, extras,
                                              self._force_spec(boundary_force_outputs))
        if macroscopic_outputs is not None:
            return self._observed_timestep_op(int(num_time_steps), macroscopic_outputs, extras)
        torch = _torch()
        step = self
        T = int(num_time_steps)
        adj = {f.name: self._adjoint_name(f) for f in extras}

        class LbmTimesteps(torch.autograd.Function):
            @staticmethod
            def forward(ctx, pdfs, *xs):
                if len(xs) != len(extras):
                    raise TypeError(f'{LbmTimesteps.__name__}.apply(pdfs, {", ".join(f.name for f in extras)}): '
                                    f'{1 + len(xs)} tensors given')
                # additional input fields (a per-cell force): constant over the steps, bound to every launch
                ex = {f.name: step._field_layout(f, x.detach()) for f, x in zip(extras, xs)}
                ctx.extras = ex
                if not step._gpu:
                    ex = {n: x.cpu().numpy() for n, x in ex.items()}
                    ctx.extras = ex
                    step.set_pdfs(pdfs.detach().cpu().numpy())
                    step.run(T, record=True, extra=ex)
                    ctx.records = step._records
                    step._records = None
                    return torch.from_numpy(step.pdf_array.copy())
                # states on fresh arrays: the input is the first state (the lattice kernels read any strides;
                # the AutoDiffOp kernels need the field's layout — ``empty_pdfs`` — or get a copy), the output, in
                # the field's layout, the last; the lattice schedule keeps the states between in the
                # row-interleaved layout, all in one allocation (no copies either way)
                lattice = step._lattice is not None
                x0 = pdfs.detach()
                x0 = x0 if lattice and step._lattice_input_ok(x0) else step._as_layout(x0)
                if lattice:
                    states = [x0] + step._internal_states(T - 1) + [step._alloc(zero=False)]
                    _lattice_sweeps(step, 'fwd', [(states[t], states[t + 1]) for t in range(T)], step._field_args(ex))
                else:
                    states = [x0]
                    for t in range(T):
                        out = step._alloc(zero=False)
                        step._fwd(states[-1], out, ex)
                        states.append(out)
                # state 0 may be the caller's tensor: keep it through save_for_backward, so that an in-place
                # change between forward and backward raises (version counter) instead of skewing the adjoint
                ctx.input_is_state0 = states[0].data_ptr() == pdfs.data_ptr()
                ctx.save_for_backward(pdfs if ctx.input_is_state0 else None)
                ctx.records = states[1:-1] if ctx.input_is_state0 else states[:-1]
                return states[-1]

            @staticmethod
            def backward(ctx, grad):
                ex = ctx.extras
                ctx.extras = None
                if not step._gpu:
                    step._records = ctx.records
                    step.set_adjoint_pdfs(grad.detach().cpu().numpy())
                    acc = {n: np.zeros_like(x) for n, x in ex.items()}
                    for t in range(T):
                        # each step's adjoint of the additional fields into a zeroed array, summed over the steps
                        tmp = {adj[n]: np.zeros_like(x) for n, x in ex.items()}
                        step.backward_time_step(step._records[-1 - t], ex, tmp)
                        for n in acc:
                            acc[n] += tmp[adj[n]]
                    step._records = step._records[:len(step._records) - T]
                    ctx.records = None
                    return (torch.from_numpy(step.adjoint_pdf_array.copy()),
                            *[torch.from_numpy(acc[f.name]) for f in extras])
                lattice = step._lattice is not None
                g = grad if lattice and step._lattice_input_ok(grad) else step._as_layout(grad)
                x0 = ctx.saved_tensors[0].detach() if ctx.input_is_state0 else None
                records = ([x0 if lattice and step._lattice_input_ok(x0) else step._as_layout(x0)]
                           if ctx.input_is_state0 else []) + list(ctx.records)
                ctx.records = None
                if lattice:
                    # adjoints of states T-1 .. 1 alternate between two row-interleaved arrays; the gradient
                    # (adjoint of state 0) leaves in the field's layout
                    out = step._alloc(zero=False)
                    launches = step._adjoint_launches(records, g, step._internal_states(min(2, T - 1)), out)
                    if not extras:
                        _lattice_sweeps(step, 'adj', launches)
                        return out
                    # the force / ω / σ adjoint: every step's adjoint launch adds its share into one array, zeroed
                    # once
                    dex, fields = step._zeroed_field_adjoints(ex, extras, torch.zeros_like)
                    _lattice_sweeps(step, 'adj', launches, fields)
                    return (out, *[dex[f.name] for f in extras])
                cur = g
                acc = {n: torch.zeros_like(x) for n, x in ex.items()}
                for t in reversed(range(T)):
                    nxt = step._alloc(zero=False)
                    tmp = {adj[n]: torch.zeros_like(x) for n, x in ex.items()}
                    step._bwd(records[t], cur, nxt, ex, tmp)
                    for n in acc:
                        acc[n] += tmp[adj[n]]
                    cur = nxt
                return (cur, *[acc[f.name] for f in extras]) if extras else cur

        LbmTimesteps.num_time_steps = T
        LbmTimesteps.lb_step = self
        return LbmTimesteps

    def _observed_timestep_op(self, T, every, extras, forces=()):
        """The time-step op that also returns the density and the velocity of every ``every``-th state
        (``create_timestep_op(macroscopic_outputs=…)``): ``Op.apply(pdfs, *extras)`` → ``(pdfs, rho, vel)``.

        The launches of the observed steps run the lattice kernels' density / velocity variant — the forward cell
        stores ρ and u of the state it writes (the compute type: float32 for float16 pdfs; 0 in obstacle cells), the
        adjoint cell adds the seeds to ``g`` where it loads it — and every other launch the plain kernels.
        ``rho [n, *domain]`` and ``vel [n, *domain, D]`` (stored component-first, a permuted view) are one
        uninitialised allocation each. Backward takes ``(grad_pdfs, grad_rho, grad_vel)``, any of them None (both
        observable gradients None: the plain adjoint kernels throughout); an observable's gradient in the layout the
        op returned is read in place, any other gets one copy.

        ``forces`` (``create_timestep_op(boundary_force_outputs=…)``, a list of ``(boundary, k)``): one more output
        ``force [T // k, D]`` per entry, after the others; ``every`` None: no density / velocity outputs. The force
        launches run after the sweeps on the recorded states (and on the output state when T is observed). Backward:
        before the adjoint launch that reads the adjoint of state t, the seeds of the forces observed at t are added
        into that array on the boundary's links (the caller's ``grad``: copied once first); a force gradient that is
        None launches nothing."""
        if self._lattice is None:
            raise NotImplementedError(
                'macroscopic_outputs / boundary_force_outputs: the density / velocity outputs are written by the lattice '
                'kernels, and this rule is not on the lattice schedule (it runs on the AutoDiffOp kernels: a rule not made by '
                'create_lb_update_rule, time-constant or other additional fields, a symbolic rate or force the '
                'lattice kernels do not take, or PSAD_LBM_LATTICE=0)')
        if every is not None and (isinstance(every, float) or int(every) < 1):
            raise ValueError(f'macroscopic_outputs: True or an int k >= 1, got {every!r}')
        torch = _torch()
        observed = every is not None
        step, k, gpu = self, int(every) if observed else 1, self._gpu
        n, D, dims = T // k if observed else 0, len(self.domain_size), list(self.domain_size)
        slot = {j * k - 1: j - 1 for j in range(1, n + 1)}          # launch t (its output: state t + 1) → slot
        forces = list(forces)
        WF = self._wall_force_kernels() if forces else None
        pdt = np.dtype(self.pdf_field.dtype.numpy_dtype)
        cdt = getattr(torch, 'float64' if pdt == np.float64 else 'float32')     # the kernels' compute type
        view = (0,) + tuple(range(2, D + 2)) + (1,)                 # [n, D, *domain] → [n, *domain, D]

        def arrays(t):
            """What the kernels take: the tensor itself, on the C target its memory as a numpy array."""
            return t if gpu else t.numpy()

        def as_returned(g, like):
            """The gradient ``g`` of an output ``like``: itself if it has that layout, else one copy in it."""
            if g is None:
                return torch.zeros_like(like)           # (preserves the strides: dense, non-overlapping)
            g = g.detach()
            if g.dtype == like.dtype and g.device == like.device and tuple(g.shape) == tuple(like.shape) and \
                    tuple(g.stride()) == tuple(like.stride()):
                return g
            out = torch.empty_like(like)
            out.copy_(g)
            return out

        class LbmTimestepsObserved(torch.autograd.Function):
            @staticmethod
            def forward(ctx, pdfs, *xs):
                if len(xs) != len(extras):
                    raise TypeError(f'{LbmTimestepsObserved.__name__}.apply(pdfs, {", ".join(f.name for f in extras)}): '
                                    f'{1 + len(xs)} tensors given')
                ex = {f.name: step._field_layout(f, x.detach()) for f, x in zip(extras, xs)}
                if not gpu:
                    ex = {name: x.cpu().numpy() for name, x in ex.items()}
                ctx.extras = ex
                x0 = pdfs.detach()
                if gpu:
                    x0 = x0 if step._lattice_input_ok(x0) else step._as_layout(x0)
                    states = [x0] + step._internal_states(T - 1) + [step._alloc(zero=False)]
                    dev = x0.device
                else:
                    states = [np.asarray(x0.cpu().numpy(), dtype=pdt)] + [step._alloc(zero=False) for _ in range(T)]
                    dev = 'cpu'
                rho = torch.empty([n] + dims, dtype=cdt, device=dev) if observed else None
                vel = torch.empty([n, D] + dims, dtype=cdt, device=dev).permute(*view) if observed else None
                macro = [None] * T
                for t, j in slot.items():
                    macro[t] = dict(rho_out=arrays(rho[j]), vel_out=arrays(vel[j]))
                _lattice_sweeps(step, 'fwd', [(states[t], states[t + 1]) for t in range(T)], step._field_args(ex),
                                macro=macro)
                ctx.input_is_state0 = gpu and states[0].data_ptr() == pdfs.data_ptr()
                ctx.records = states[1:-1] if ctx.input_is_state0 else states[:-1]
                out = states[-1] if gpu else torch.from_numpy(states[-1])
                # (the outputs are what a compressible rule's adjoint reads: saved, so that an in-place change between
                # forward and backward raises)
                ctx.save_for_backward(pdfs if ctx.input_is_state0 else None, rho, vel)
                ctx.set_materialize_grads(False)
                # the boundary forces of the observed states: launches on the states where they lie (no copies); the
                # link lists as they are now, kept for the backward
                fout, ctx.force_links = [], []
                for b, kf in forces:
                    links = step.boundary_links(b)
                    ctx.force_links.append(links)
                    Fo = torch.empty([T // kf, D], dtype=cdt, device=dev)
                    for j in range(T // kf):
                        WF.force(states[(j + 1) * kf], links, out=arrays(Fo[j]))
                    fout.append(Fo)
                return (out, rho, vel, *fout) if observed else (out, *fout)

            @staticmethod
            def backward(ctx, grad, *more):
                grad_rho, grad_vel = more[:2] if observed else (None, None)
                grad_forces = more[2:] if observed else more
                ex = ctx.extras
                ctx.extras = None
                x0, rho, vel = ctx.saved_tensors
                if observed:
                    rho, vel = rho.detach(), vel.detach()
                # state t → [(links, dF)] of the forces observed there whose gradient arrived
                seeds = {}
                for (b, kf), links, gF in zip(forces, ctx.force_links, grad_forces):
                    if gF is None or links.n == 0:
                        continue
                    gF = gF.detach().to(cdt).contiguous()
                    for j in range(T // kf):
                        seeds.setdefault((j + 1) * kf, []).append((links, arrays(gF[j] if gpu else gF[j].cpu())))
                ctx.force_links = None
                if grad is None:
                    g = step._alloc(zero=True)
                elif gpu:
                    g = grad if step._lattice_input_ok(grad) else step._as_layout(grad)
                else:
                    g = np.asarray(grad.detach().cpu().numpy(), dtype=pdt)
                if T in seeds and grad is not None and (
                        g.data_ptr() == grad.data_ptr() if gpu else np.shares_memory(g, grad.detach().cpu().numpy())):
                    # the seed of F(s_T) goes into the adjoint of state T: not into the caller's tensor
                    g = g.clone() if gpu else g.copy()
                records = list(ctx.records)
                if ctx.input_is_state0:
                    x0 = x0.detach()
                    records = [x0 if step._lattice_input_ok(x0) else step._as_layout(x0)] + records
                ctx.records = None
                ping = step._internal_states(min(2, T - 1)) if gpu else \
                    [step._alloc(zero=False) for _ in range(min(2, T - 1))]
                out = step._alloc(zero=False)
                launches, macro, before = step._adjoint_launches(records, g, ping, out), [], []
                seeded = grad_rho is not None or grad_vel is not None
                if seeded:
                    drho, dvel = as_returned(grad_rho, rho), as_returned(grad_vel, vel)
                for t, (_, cur, _) in zip(reversed(range(T)), launches):
                    # (this launch reads ``cur``, the adjoint of state t + 1)
                    before.append(None if t + 1 not in seeds else
                                  (lambda a=cur, ls=seeds[t + 1]: [WF.adjoint(a, links, dF) for links, dF in ls]))
                    j = slot.get(t) if seeded else None
                    macro.append(None if j is None else dict(rho_out=arrays(rho[j]), vel_out=arrays(vel[j]),
                                                             drho=arrays(drho[j]), dvel=arrays(dvel[j])))
                # the force / ω / σ adjoint: every step's adjoint launch adds its share into one array, zeroed once
                dex, fields = step._zeroed_field_adjoints(ex, extras, torch.zeros_like if gpu else np.zeros_like)
                _lattice_sweeps(step, 'adj', launches, fields, macro=macro, before=before if seeds else None)
                if not gpu:
                    return (torch.from_numpy(out), *[torch.from_numpy(dex[f.name]) for f in extras])
                return (out, *[dex[f.name] for f in extras])

        LbmTimestepsObserved.num_time_steps = T
        LbmTimestepsObserved.lb_step = self
        LbmTimestepsObserved.observed_states = tuple(j * k for j in range(1, n + 1))
        LbmTimestepsObserved.boundary_force_states = tuple(tuple(j * kf for j in range(1, T // kf + 1))
                                                           for _, kf in forces)
        return LbmTimestepsObserved

    def _field_layout(self, f, t):
        """An additional input tensor in field ``f``'s memory layout (fzyx: components-first) on the step's side."""
        if not self._gpu:
            # (a scalar field may arrive as an expanded scalar, stride 0: its adjoint array needs cells of its own)
            return t if f.index_dimensions else t.contiguous()
        if f.index_dimensions and f.is_soa:
            from ..zslab import ZSlabOp
            return ZSlabOp._layout(f, t)
        return t.contiguous()

    def _pdf_io_field(self):
        """The pdf field of the macroscopic ops, in the step's pdf layout (fzyx pdfs enter without a copy)."""
        return ps.fields(f"pdfs({self.method.Q}): {np.dtype(self.pdf_field.dtype.numpy_dtype).name}"
                         f"[{len(self.domain_size)}D]", layout='fzyx' if self.pdf_field.is_soa else None)

    def create_end_to_end_op(self, num_time_steps, velocity_input_tensor, density_input_tensor,
                             additional_fields_to_tensor_map=None, force_input_tensor=None, backend='torch_native',
                             num_times_steps_without_save=0, macroscopic_outputs=False, boundary_force_outputs=None,
                             **kernel_compilation_kwargs):
        """Equilibrium from (ρ, u) → ``num_time_steps`` steps → (ρ, u), differentiable end to end
        (``_autodiff_lbstep.py:310-334``, there TensorFlow only): the setter op, the time-step ops in groups of
        ``num_times_steps_without_save + 1`` steps, the getter op, evaluated on the given tensors (torch
        autograd records the chain). Returns ``SimulationResultsTensors``. ``macroscopic_outputs``: every group is
        observed at its end (``create_timestep_op(group, macroscopic_outputs=group)``) and the result also carries
        ``density_trajectory`` ``[groups, *domain]`` and ``velocity_trajectory`` ``[groups, *domain, D]``.
        ``boundary_force_outputs`` (a boundary or a list of boundaries set on the step): the force on each at every
        group's end, ``boundary_force_trajectory`` ``[groups, D]`` (a list of those for a list; a ``(boundary, k)`` pair is
        accepted with k = 1 only)."""
        if str(backend).lower() not in ('torch_native', 'torch'):
            raise NotImplementedError(f"backend '{backend}': only the torch backends are built")
        from ._method import force_is_field
        given = {getattr(f, 'name', f): t for f, t in dict(additional_fields_to_tensor_map or {}).items()}
        force = getattr(self._update_rule, 'force', None)
        if force_input_tensor is not None:
            if not force_is_field(force):
                raise ValueError('force_input_tensor given, but the update rule has no force field')
            (ff,) = {a.field for v in force for a in sp.sympify(v).atoms(ps.Field.Access)}
            given[ff.name] = force_input_tensor
        missing = [f.name for f in self._additional_fields if f.name not in given]
        if missing:
            raise ValueError(f'tensors for the update rule\'s additional input fields {missing} are needed '
                             '(additional_fields_to_tensor_map / force_input_tensor)')
        xs = [given[f.name] for f in self._additional_fields]
        setter = self._e2e_ops.get('setter') if hasattr(self, '_e2e_ops') else None
        if setter is None:
            self._e2e_ops = {'setter': self.create_macroscopic_setter_op(backend, **kernel_compilation_kwargs),
                             'getter': self.create_macroscopic_getter_op(backend, **kernel_compilation_kwargs)}
        ops = self._e2e_ops
        group = int(num_times_steps_without_save) + 1
        bodies = None
        if boundary_force_outputs is not None:
            # (a boundary, a (boundary, 1) pair or a list of those, as the time-step op parses them; every group is
            # observed at its end, so another k has no meaning here)
            spec = self._force_spec(boundary_force_outputs)
            if any(k != 1 for _, k in spec):
                raise ValueError('create_end_to_end_op(boundary_force_outputs=…): boundaries, not (boundary, k) pairs '
                                 'with k > 1 — the force is taken at the end of every group of '
                                 'num_times_steps_without_save + 1 steps')
            bodies = [b for b, _ in spec]
        step_op = self.create_timestep_op(group, backend=backend,
                                          macroscopic_outputs=group if macroscopic_outputs else None,
                                          boundary_force_outputs=None if bodies is None else [(b, group) for b in bodies])
        (input_pdf,) = ops['setter'].apply(density_input_tensor, velocity_input_tensor)
        out = input_pdf
        trajectory = []
        force_trajectory = []
        for _ in range(int(num_time_steps) // group):
            if macroscopic_outputs or bodies is not None:
                out, *observed = step_op.apply(out, *xs)
                if macroscopic_outputs:
                    trajectory.append(observed[:2])
                force_trajectory.append(observed[2 if macroscopic_outputs else 0:])
            else:
                out = step_op.apply(out, *xs)
        rho, vel = self._apply_getter(ops['getter'], out, given)
        result = SimulationResultsTensors(input_pdf, out, rho, vel)
        if macroscopic_outputs:
            torch = _torch()
            result.density_trajectory = torch.cat([r for r, _ in trajectory]) if trajectory else None
            result.velocity_trajectory = torch.cat([v for _, v in trajectory]) if trajectory else None
        if bodies is not None:
            torch = _torch()
            per_body = [torch.cat([fs[i] for fs in force_trajectory]) if force_trajectory else None
                        for i in range(len(bodies))]
            result.boundary_force_trajectory = per_body if isinstance(boundary_force_outputs, list) or \
                len(per_body) > 1 else per_body[0]
        return result

    def _macroscopic_fields(self):
        dt = self.pdf_field.dtype.numpy_dtype
        D = len(self.domain_size)
        return ps.fields(f"rho, vel({D}): {np.dtype(dt).name}[{D}D]")

    def _apply_getter(self, getter, pdfs, given):
        """The getter on ``pdfs`` (and, with a per-cell Guo force, the force tensor: its inputs in the op's order)."""
        names = [f.name for f in getter.autodiff_op.forward_input_fields]
        pdf = self._pdf_io_field().name
        return getter.apply(*[pdfs if n == pdf else given[n] for n in names])

    def create_macroscopic_getter_op(self, backend='torch_native', **kernel_compilation_kwargs):
        """ρ and u from pdfs as a differentiable op (``_autodiff_lbstep.py:249-280``): ``Op.apply(pdfs)`` →
        ``(rho, vel)`` (a per-cell Guo force: its field is an input too, in the op's ``forward_input_fields``
        order)."""
        from ._method import macroscopic_getter
        rho, vel = self._macroscopic_fields()
        pdf = self._pdf_io_field()
        ac = macroscopic_getter(self.method, pdf, rho, vel, getattr(self._update_rule, 'compressible', False),
                                getattr(self._update_rule, 'force_model', None), getattr(self._update_rule, 'force', None),
                                zero_centered=getattr(self._update_rule, 'zero_centered', False))
        op = AutoDiffOp(ac, 'LBM_GetMacroscopicValues', diff_mode='transposed', **kernel_compilation_kwargs)
        return op.create_tensorflow_op(use_cuda=self._gpu, backend=backend)

    def create_macroscopic_setter_op(self, backend='torch_native', **kernel_compilation_kwargs):
        """pdfs = feq(ρ, u) as a differentiable op (``_autodiff_lbstep.py:282-308``): ``Op.apply(rho, vel)``."""
        from ._method import equilibrium_setter
        rho, vel = self._macroscopic_fields()
        pdf = self._pdf_io_field()
        ac = equilibrium_setter(self.method, pdf, rho, vel, getattr(self._update_rule, 'compressible', False),
                                zero_centered=getattr(self._update_rule, 'zero_centered', False))
        op = AutoDiffOp(ac, 'LBM_SetMacroscopicValues', diff_mode='transposed', **kernel_compilation_kwargs)
        return op.create_tensorflow_op(use_cuda=self._gpu, backend=backend)
