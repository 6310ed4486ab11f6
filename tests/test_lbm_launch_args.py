"""The VALUES the lattice launcher packs into a kernel's argument buffer, by argument name.

The emitted sources' shas pin each kernel's parameter list; what the host puts into every slot — which array's pointer,
whose strides — is checked here, on CPU tensors (``LatticeKernels._values``, ``struct_format`` and ``_pack`` read
shapes, strides and addresses only; no kernel runs). Every array of a launch has strides of its own, so a pointer or a
stride block bound to another operand's shows."""
import functools
import itertools
import struct

import numpy as np
import pytest
import torch

from pystencils_autodiff_amd import lbm
from pystencils_autodiff_amd.lbm import _lattice_kernels as LK
from pystencils_autodiff_amd.lbm._lattice_source import struct_format

OMEGA = 1.25        # (a float32 exactly)
LATTICES = {'D2Q9': ((3, 5), 'int'), 'D3Q19': ((2, 3, 5), 'long long')}      # stencil → (domain, stride type)


@functools.lru_cache(maxsize=None)
def _kernels(stencil, force, omega, solid):
    kw = dict(force_model='guo', force_field=True) if force else {}
    return LK.LatticeKernels(lbm.LBStencil(stencil), True, np.dtype('float32'), True, 'gpu', omega_field=omega,
                             solid_field=solid, **kw)


def _view(dom, order, pad=0, last=None):
    """A float32 view of shape ``dom`` (+ ``(last,)``) whose axes lie in memory in the order ``order`` (positions in the
    shape, slowest first), the fastest of them padded by ``pad`` elements: a stride pattern per (order, pad)."""
    shape = list(dom) + ([last] if last else [])
    mem = [shape[a] for a in order]
    mem[-1] += pad
    inverse = [order.index(a) for a in range(len(shape))]
    return torch.zeros(mem).permute(*inverse)[tuple(slice(0, n) for n in shape)]


def _like(t):
    """Another array with ``t``'s shape and strides (an adjoint beside its field)."""
    return torch.empty_strided(tuple(t.shape), tuple(t.stride()))


def _strides(prefix, axes, t, D):
    """name → value of the stride arguments ``{prefix}_{axis}`` of ``t`` (``[*domain]``, or ``[*domain, n]`` with the
    leading axis letter the last dimension's); the z stride of a 2-D lattice is 0."""
    st = list(t.stride())
    lead = [st[D]] if len(axes) == 4 else []
    return dict(zip((f'{prefix}_{a}' for a in axes), lead + [0] * (3 - D) + st[:D]))


def _bytes(t):
    return (sum(s * (n - 1) for s, n in zip(t.stride(), t.shape)) + 1) * t.element_size()


@pytest.mark.parametrize('force,omega,solid', list(itertools.product((False, True), repeat=3)))
@pytest.mark.parametrize('macro', [False, True])
@pytest.mark.parametrize('which', ['fwd', 'adj'])
@pytest.mark.parametrize('stencil', sorted(LATTICES))
def test_packed_argument_values(stencil, which, macro, force, omega, solid):
    """``forward`` / ``adjoint``'s keywords → the packed buffer of ``lbm_fwd`` / ``lbm_adj``: unpacked by the kernel's
    table, the buffer holds exactly the expected arguments, and each — pointer, stride, extent, reach, rate — has the
    value computed here from the tensor it belongs to."""
    dom, idx = LATTICES[stencil]
    D, K = len(dom), _kernels(stencil, force, omega, solid)
    Q, sp = K.stencil.Q, list(range(len(dom)))
    # the pdf arrays: fzyx, AoS, row-interleaved, padded AoS
    layouts = dict(src=([D] + sp, 0), dst=(sp + [D], 0), g=(sp[:-1] + [D, D - 1], 0), out=(sp + [D], 2))
    pdfs = {n: _view(dom, *layouts[n], last=Q) for n in (('src', 'dst') if which == 'fwd' else ('src', 'g', 'out'))}
    mask = torch.zeros(dom, dtype=torch.int32)
    F = _view(dom, [D] + sp, 1, last=D)                     # a permuted fzyx force (padded rows)
    W = _view(dom, sp[::-1])                                # a transposed ω view
    S = _view(dom, sp, 3)                                   # a sliced σ view of another pitch
    dF, dW, dS = _like(F), _like(W), _like(S)
    rho, vel = _view(dom, sp, 4), _view(dom, [D] + sp, 5, last=D)
    drho, dvel = _like(rho), _like(vel)
    arrays = list(pdfs.values()) + [F, W, S, rho, vel]
    assert len({tuple(t.stride()) for t in arrays}) == len(arrays)          # (the premise: no two alike)
    assert len({t.data_ptr() for t in arrays + [dF, dW, dS, drho, dvel, mask]}) == len(arrays) + 6

    # the launch, through the keyword API; ``run`` is where a launch would build its plan from these operands
    calls = []
    K.run = lambda *a: calls.append(a)
    try:
        kw = dict(force=F if force else None, omf=W if omega else None, sof=S if solid else None)
        if which == 'fwd':
            K.forward(*pdfs.values(), OMEGA, mask, **kw, **(dict(rho_out=rho, vel_out=vel) if macro else {}))
        else:
            kw.update(dforce=dF if force else None, domf=dW if omega else None, dsof=dS if solid else None)
            K.adjoint(*pdfs.values(), OMEGA, mask, **kw,
                      **(dict(rho_out=rho, vel_out=vel, drho=drho, dvel=dvel) if macro else {}))
    finally:
        del K.run
    (kind, tensors, om, m, ids, fields, marr, cells, stream), = calls
    assert kind == which and ids is None and cells is None and stream is None and bool(marr) == macro
    table = K.table(which, macro)
    fmt = struct_format(table, idx, K.ct)
    ops = K.operands(tensors, m, ids, fields, macro=marr)
    buf = LK._pack(fmt, *K._values(table, ops, om))
    got = {a.name: struct.unpack_from('<' + c, buf, LK._offset(fmt, i))[0] for i, (a, c) in enumerate(zip(table, fmt))}
    assert len(got) == len(table)

    # what the buffer must hold, from the tensors themselves
    want = {n: t.data_ptr() for n, t in pdfs.items()}
    want.update(nbmask=mask.data_ptr(), wallid=0, **dict(zip('ZYX', (1,) * (3 - D) + tuple(dom))))
    for n, t in pdfs.items():
        want.update(_strides(n[0], 'qzyx', t, D))
        want[f'{n[0]}_bytes'] = _bytes(t)
    adj = which == 'adj'
    if force:
        want.update(force=F.data_ptr(), **({'dforce': dF.data_ptr()} if adj else {}), **_strides('f', 'czyx', F, D))
    if omega:
        want.update(omf=W.data_ptr(), **({'domega': dW.data_ptr()} if adj else {}), **_strides('w', 'zyx', W, D))
    if solid:
        want.update(sigf=S.data_ptr(), **({'dsolid': dS.data_ptr()} if adj else {}), **_strides('p', 'zyx', S, D))
    if macro:
        want.update(rho_out=rho.data_ptr(), vel_out=vel.data_ptr(), **({'drho': drho.data_ptr(),
                                                                        'dvel': dvel.data_ptr()} if adj else {}),
                    **_strides('r', 'zyx', rho, D), **_strides('v', 'czyx', vel, D))
    want['omega_s' if omega else 'omega'] = OMEGA
    assert sorted(got) == sorted(want)
    assert {n: (got[n], want[n]) for n in want if got[n] != want[n]} == {}
    # the pointer slots a launch patches: the table's pointers, in its order
    names = K.table_pointer_names(which, macro)
    assert K.pointers(which, ops, macro) == tuple(want[n] for n in names)
    assert struct.unpack_from(f'<{len(names)}Q', buf, 0) == tuple(want[n] for n in names)
