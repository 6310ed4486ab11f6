"""Which update rules run on the lattice schedule: ``lattice_rule`` reads a rule made by ``create_lb_update_rule`` and
returns what ``LatticeKernels`` is built from (a ``LatticeRule``), or None for a rule that runs on the ``AutoDiffOp``
kernels instead."""
import os
from types import MappingProxyType
from typing import NamedTuple

import numpy as np
import sympy as sp

from .. import ps
from ._lattice_source import CELL_FIELDS


class LatticeRule(NamedTuple):
    """What the lattice kernels of a rule are built from (``AutoDiffLatticeBoltzmannStep._lattice_kernels``).
    ``force_model`` / ``force``: the force term and its D constants (None: no force, or a force field); ``trt``:
    None, ``('magic', Λ)`` or ``('rate', ω₋)``; ``mrt``: None or the matrices ``(P_ω, C)``; ``smagorinsky``: None or
    C_s; ``fields``: per kind of ``CELL_FIELDS`` the rule's field read per cell, or None; ``rate``: where the scalar ω
    argument comes from — ``('field', None)`` (unused: the kernels read the ω field), ``('param', name)`` (the step's
    ``kernel_params``) or ``('number', value)`` (made a float per launch)."""
    force_model: object
    force: object
    trt: object
    mrt: object
    smagorinsky: object
    fields: object
    rate: tuple


def _plain_vector_field(expr, D):
    """The FIELD when ``expr`` is exactly ``F(x)[a]`` per axis a (one field of D components read at the cell
    itself), else None."""
    if expr is None:
        return None
    comps = [sp.sympify(v) for v in expr]
    if len(comps) != D or not all(isinstance(c, ps.Field.Access) for c in comps):
        return None
    fields = {c.field for c in comps}
    if len(fields) != 1:
        return None
    (F,) = fields
    if F.index_dimensions != 1 or int(F.index_shape[0]) != D:
        return None
    for a, c in enumerate(comps):
        if tuple(int(o) for o in c.offsets) != (0,) * D or tuple(int(i) for i in c.index) != (a,):
            return None
    return F


def _plain_scalar_field(expr, D, dtype):
    """The FIELD when ``expr`` is exactly ``w(x)``: a scalar field (no index dimension) of the pdf dtype read at the
    cell itself, else None."""
    if not isinstance(expr, ps.Field.Access):
        return None
    w = expr.field
    if w.index_dimensions != 0 or w.spatial_dimensions != D or tuple(int(o) for o in expr.offsets) != (0,) * D:
        return None
    return w if np.dtype(w.dtype.numpy_dtype) == np.dtype(dtype) else None


def plain_cell_fields(update_rule, src):
    """Per kind of ``CELL_FIELDS`` the field the lattice kernels can take as an array, accumulating its adjoint: the
    rule's force read as ``F(x)[a]`` (the field's centre, component a, for every axis), its rate as ``w(x)`` and its
    solid fraction as ``s(x)`` (scalar fields of the pdf dtype at the cell itself); None for any other expression (a
    number, a symbol, 1/(3 ν(x) + 1/2), an offset read, another dtype), which runs on the AutoDiffOp kernels."""
    D, dtype = src.spatial_dimensions, src.dtype.numpy_dtype
    return {f.kind: _plain_vector_field(getattr(update_rule, f.rule, None), D) if f.vector else
            _plain_scalar_field(getattr(update_rule, f.rule, None), D, dtype) for f in CELL_FIELDS}


def lattice_rule(update_rule, src, time_constant_fields):
    """The ``LatticeRule`` of ``update_rule`` (``src``: its pdf field) if it runs on the lattice schedule — a rule of
    ``create_lb_update_rule`` (SRT / TRT / MRT, stream_pull_collide) whose additional inputs are per-cell fields the
    kernels take — else None. (``PSAD_LBM_LATTICE=0``, read here: None, the AutoDiffOp kernels instead — tests of that
    path, A/B probes.)"""
    dtype = np.dtype(src.dtype.numpy_dtype)
    # the fields the rule reads beside its pdfs (what the step takes as additional inputs)
    read = {a.field for asg in update_rule.all_assignments for a in sp.sympify(asg.rhs).atoms(ps.Field.Access)}
    written = {asg.lhs.field for asg in update_rule.all_assignments if isinstance(asg.lhs, ps.Field.Access)}
    additional = read - {src} - written
    rr = getattr(update_rule, 'relaxation_rate', None)
    fields = plain_cell_fields(update_rule, src)
    # the scalar ω argument: unused with a per-cell rate w(x); no lattice kernels for any other rate that reads a field
    if fields['omega'] is not None:
        rate = ('field', None)
    elif rr is None or sp.sympify(rr).atoms(ps.Field.Access):
        rate = None
    else:
        rate = ('param', rr.name) if isinstance(rr, sp.Symbol) else ('number', rr)
    # the force: a plain per-cell field, D numbers or none
    force = getattr(update_rule, 'force', None)
    force_model = getattr(update_rule, 'force_model', None)
    if fields['force'] is not None:
        lattice_force = (force_model, None)
    elif force is None or all(sp.sympify(v).is_number for v in force):
        lattice_force = (force_model, None if force is None else tuple(float(v) for v in force))
    else:
        lattice_force = None
    # a solid fraction that is not a plain field (a number, a symbol, …): the AutoDiffOp kernels
    solid_ok = getattr(update_rule, 'solid_fraction', None) is None or fields['solid'] is not None
    extras_ok = additional == {f for f in fields.values() if f is not None}
    # TRT: the odd rate from the magic number (a function of the ω argument) or a constant
    trt, trt_ok = None, True
    if getattr(update_rule, 'method', 'srt') == 'trt':
        if getattr(update_rule, 'magic_number', None) is not None:
            trt = ('magic', float(update_rule.magic_number))
        elif sp.sympify(update_rule.relaxation_rate_odd).is_number:
            trt = ('rate', float(update_rule.relaxation_rate_odd))
        else:
            trt_ok = False                      # a symbolic odd rate: the AutoDiffOp kernels
    # MRT: the relaxation matrix A = ω P_ω + C (groups relaxing with the rule's ω / with constant rates)
    mrt = None
    if getattr(update_rule, 'method', 'srt') == 'mrt':
        from ._method import MRT_GROUPS, mrt_relaxation_matrices
        P = mrt_relaxation_matrices(update_rule.stencil)
        Qn = update_rule.stencil.Q
        Pw = [[0.0] * Qn for _ in range(Qn)]
        Cm = [[0.0] * Qn for _ in range(Qn)]
        om = sp.sympify(update_rule.relaxation_rate)
        for grp in MRT_GROUPS:
            r = sp.sympify(update_rule.mrt_rates[grp])
            if r == om:
                tgt, scale = Pw, 1.0
            elif r.is_number:
                tgt, scale = Cm, float(r)
            else:
                trt_ok = False                  # a symbolic rate other than ω: the AutoDiffOp kernels
                break
            for i in range(Qn):
                for k in range(Qn):
                    tgt[i][k] += scale * float(P[grp][i][k])
        else:
            mrt = (Pw, Cm)
    # Smagorinsky: a numeric C_s is a constant of the lattice kernels; a symbolic one, float16 pdfs or a per-cell
    # force field (its adjoint would need ∂ω_eff/∂F) run on the AutoDiffOp kernels
    cs = getattr(update_rule, 'smagorinsky', None)
    smagorinsky = float(cs) if cs is not None and sp.sympify(cs).is_number else None
    smag_ok = cs is None or (smagorinsky is not None and fields['force'] is None and dtype != np.float16)
    if not (getattr(update_rule, 'stencil', None) is not None and not time_constant_fields
            and lattice_force is not None and smag_ok
            and os.environ.get('PSAD_LBM_LATTICE', '1') != '0'
            and extras_ok and solid_ok and trt_ok and rate is not None
            and dtype in (np.float16, np.float32, np.float64)
            # (float16 pdfs with a force / ω / σ field: the AutoDiffOp kernels — the lattice kernels would accumulate
            # the field's adjoint over the steps in float16)
            and (dtype != np.float16 or all(f is None for f in fields.values()))
            and (fields['force'] is None or fields['force'].dtype.numpy_dtype == src.dtype.numpy_dtype)):
        return None
    return LatticeRule(*lattice_force, trt, mrt, smagorinsky, MappingProxyType(fields), rate)
