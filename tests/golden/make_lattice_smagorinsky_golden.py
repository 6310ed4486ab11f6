"""Generate ``tests/golden/lattice_smagorinsky_source_sha.json`` (run: python
tests/golden/make_lattice_smagorinsky_golden.py): the sha256 of every emitted source of the lattice Boltzmann kernels'
Smagorinsky variants — the C target, and the HIP module for both index types in both addressing modes (with link
programs: the main and the fix-up module). Nothing is compiled. The sources without the model are pinned by
``lattice_source_sha*.json`` and ``lattice_fp16_source_sha.json``; ``tests/test_lbm_smagorinsky.py`` compares ``shas()``
with this file.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import sympy as sp  # noqa: E402

from pystencils_autodiff_amd import lbm, ps  # noqa: E402

PATH = os.path.join(HERE, 'lattice_smagorinsky_source_sha.json')
CS = 0.2

# name → (stencil, domain, method, compressible, force model, walls, layout, ω field, zero-centred)
LATTICES = {
    'D2Q9-srt-periodic': ('D2Q9', (8, 6), 'srt', True, None, None, 'fzyx', False, False),
    'D2Q9-srt-periodic-incompressible-zc': ('D2Q9', (8, 6), 'srt', False, None, None, 'fzyx', False, True),
    'D2Q9-srt-noslip-omega-field': ('D2Q9', (8, 6), 'srt', True, None, 'channel', 'fzyx', True, False),
    'D2Q9-srt-pressure': ('D2Q9', (8, 6), 'srt', True, None, 'pressure', 'numpy', False, False),
    'D2Q9-trt-periodic-guo': ('D2Q9', (8, 6), 'trt', False, 'guo', None, 'fzyx', False, False),
    'D2Q9-mrt-periodic-simple': ('D2Q9', (8, 6), 'mrt', True, 'simple', None, 'numpy', False, False),
    'D3Q19-srt-channel-guo': ('D3Q19', (8, 6, 5), 'srt', True, 'guo', 'channel', 'fzyx', False, False),
    'D3Q19-mrt-periodic-omega-field': ('D3Q19', (8, 6, 5), 'mrt', True, None, None, 'fzyx', True, False),
    'D3Q27-srt-channel': ('D3Q27', (8, 6, 5), 'srt', True, None, 'channel', 'fzyx', False, False),
}
DTYPES = ['float32', 'float64']


def kernels(name, dtype, target, cs=CS):
    """The ``LatticeKernels`` of lattice ``name`` for ``dtype`` pdfs on ``target`` ('gpu' / 'cpu')."""
    stencil, shape, method, compressible, fm, walls, layout, field, zc = LATTICES[name]
    D = len(shape)
    rate = ps.fields(f'omega_f: {dtype}[{D}D]').center if field else sp.Symbol('omega')
    kw = dict(relaxation_rate=rate)
    if method == 'trt':
        kw.update(method='trt')
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[rate, 1.1, 0.9, 1.2])
    if fm:
        kw.update(force_model=fm, force=(1e-3, -2e-3, 5e-4)[:D])
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, layout=layout,
                                     zero_centered=zc, smagorinsky=cs, **kw)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=None if field else 1.3,
                                            target=target)
    if walls in ('channel', 'pressure'):
        step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, 0])
        step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, -1])
    if walls == 'pressure':
        step.set_boundary_including_adjoint(lbm.FixedDensity(1.01, name='inlet'), lbm.make_slice[0, 1:-1])
        step.set_boundary_including_adjoint(lbm.FixedDensity(0.99, name='outlet'), lbm.make_slice[-1, 1:-1])
    assert step._lattice is not None
    return step._lattice_kernels()


def shas():
    def sha(s):
        return hashlib.sha256(s.encode()).hexdigest()
    out = {}
    for name in LATTICES:
        for dtype in DTYPES:
            key = f'{name}/{dtype}'
            out[f'{key}/c'] = sha(kernels(name, dtype, 'cpu').source())
            K = kernels(name, dtype, 'gpu')
            for idx in ('int', 'long long'):
                for addr in ('buf', 'ptr'):
                    for fix in ((False, True) if K.programs is not None else (False,)):
                        out[f'{key}/hip-{idx.replace(" ", "")}-{addr}{"-fix" if fix else ""}'] = \
                            sha(K.source(idx, addr, fix=fix))
    return out


if __name__ == '__main__':
    table = shas()
    with open(PATH, 'w') as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print(f'{len(table)} sources -> {PATH}')
