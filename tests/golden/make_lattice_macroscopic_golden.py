"""Generate ``tests/golden/lattice_macroscopic_source_sha.json`` (run: python
tests/golden/make_lattice_macroscopic_golden.py): the sha256 of every emitted source of the lattice Boltzmann kernels'
density / velocity variant (``LatticeSource.macroscopic``) — the C target, and the HIP module for both index types in
both addressing modes (with link programs: the main and the fix-up module). Nothing is compiled. The sources with the
flag off are pinned by ``lattice_source_sha*.json``, ``lattice_fp16_source_sha.json`` and
``lattice_smagorinsky_source_sha.json``; ``tests/test_lbm_macroscopic_outputs.py`` compares ``shas()`` with this file.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import sympy as sp  # noqa: E402

from pystencils_autodiff_amd import lbm, ps  # noqa: E402

PATH = os.path.join(HERE, 'lattice_macroscopic_source_sha.json')

# name → (stencil, domain, method, compressible, force model, force field, walls, layout, ω field, zero-centred, C_s)
LATTICES = {
    'D2Q9-srt-periodic': ('D2Q9', (8, 6), 'srt', True, None, False, None, 'fzyx', False, False, None),
    'D2Q9-srt-periodic-incompressible-zc': ('D2Q9', (8, 6), 'srt', False, None, False, None, 'fzyx', False, True,
                                            None),
    'D2Q9-srt-noslip-omega-field': ('D2Q9', (8, 6), 'srt', True, None, False, 'channel', 'fzyx', True, False, None),
    'D2Q9-srt-pressure': ('D2Q9', (8, 6), 'srt', True, None, False, 'pressure', 'numpy', False, False, None),
    'D2Q9-trt-periodic-guo': ('D2Q9', (8, 6), 'trt', False, 'guo', False, None, 'fzyx', False, False, None),
    'D2Q9-srt-periodic-guo-field': ('D2Q9', (8, 6), 'srt', True, 'guo', True, None, 'fzyx', False, False, None),
    'D2Q9-mrt-periodic-simple': ('D2Q9', (8, 6), 'mrt', True, 'simple', False, None, 'numpy', False, False, None),
    'D2Q9-srt-pressure-smagorinsky': ('D2Q9', (8, 6), 'srt', True, None, False, 'pressure', 'fzyx', False, False,
                                      0.2),
    'D3Q19-srt-channel-guo': ('D3Q19', (8, 6, 5), 'srt', True, 'guo', False, 'channel', 'fzyx', False, False, None),
    'D3Q19-srt-periodic-incompressible': ('D3Q19', (8, 6, 5), 'srt', False, None, False, None, 'fzyx', False, False,
                                          None),
    'D3Q27-srt-channel': ('D3Q27', (8, 6, 5), 'srt', True, None, False, 'channel', 'fzyx', False, False, None),
}
DTYPES = ['float32', 'float64']
HALF = ['D2Q9-srt-periodic', 'D2Q9-srt-periodic-incompressible-zc', 'D3Q27-srt-channel']     # float16 pdfs too


def kernels(name, dtype, target):
    """The ``LatticeKernels`` of lattice ``name`` for ``dtype`` pdfs on ``target`` ('gpu' / 'cpu')."""
    stencil, shape, method, compressible, fm, ffield, walls, layout, field, zc, cs = LATTICES[name]
    D = len(shape)
    rate = ps.fields(f'omega_f: {dtype}[{D}D]').center if field else sp.Symbol('omega')
    kw = dict(relaxation_rate=rate)
    if method == 'trt':
        kw.update(method='trt')
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[rate, 1.1, 0.9, 1.2])
    if fm:
        kw.update(force_model=fm, force=ps.fields(f'F({D}): {dtype}[{D}D]') if ffield else (1e-3, -2e-3, 5e-4)[:D])
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
        for dtype in DTYPES + (['float16'] if name in HALF else []):
            key = f'{name}/{dtype}'
            out[f'{key}/c'] = sha(kernels(name, dtype, 'cpu').source(macro=True))
            K = kernels(name, dtype, 'gpu')
            for idx in ('int', 'long long'):
                for addr in ('buf', 'ptr'):
                    for fix in ((False, True) if K.programs is not None else (False,)):
                        out[f'{key}/hip-{idx.replace(" ", "")}-{addr}{"-fix" if fix else ""}'] = \
                            sha(K.source(idx, addr, fix=fix, macro=True))
    return out


if __name__ == '__main__':
    table = shas()
    with open(PATH, 'w') as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print(f'{len(table)} sources -> {PATH}')
