"""Generate ``tests/golden/lattice_fp16_source_sha.json`` (run: python tests/golden/make_lattice_fp16_golden.py): the
sha256 of every emitted source of the lattice Boltzmann kernels' float16 and zero-centred variants — the C target,
and the HIP module for both index types in both addressing modes. Nothing is compiled. The plain float32 / float64
sources are pinned by ``lattice_source_sha.json`` / ``lattice_source_sha_all.json``
(``tests/test_lbm_neighbour_links.py``); ``tests/test_lbm_zero_centered.py`` compares ``shas()`` with this file.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))

import sympy as sp  # noqa: E402

from pystencils_autodiff_amd import lbm  # noqa: E402

PATH = os.path.join(HERE, 'lattice_fp16_source_sha.json')

# name → (stencil, domain, method, compressible, force model, walls, layout)
LATTICES = {
    'D2Q9-srt-periodic': ('D2Q9', (8, 6), 'srt', True, None, None, 'fzyx'),
    'D2Q9-srt-noslip': ('D2Q9', (8, 6), 'srt', True, None, 'channel', 'fzyx'),
    'D2Q9-srt-cavity': ('D2Q9', (8, 6), 'srt', True, None, 'cavity', 'numpy'),
    'D2Q9-trt-periodic-guo': ('D2Q9', (8, 6), 'trt', False, 'guo', None, 'fzyx'),
    'D2Q9-mrt-periodic-simple': ('D2Q9', (8, 6), 'mrt', True, 'simple', None, 'numpy'),
    'D3Q19-srt-channel': ('D3Q19', (8, 6, 5), 'srt', False, None, 'channel', 'fzyx'),
    'D3Q19-trt-channel-guo': ('D3Q19', (8, 6, 5), 'trt', True, 'guo', 'channel', 'fzyx'),
    'D3Q19-mrt-periodic': ('D3Q19', (8, 6, 5), 'mrt', True, None, None, 'fzyx'),
    'D3Q27-srt-channel': ('D3Q27', (8, 6, 5), 'srt', True, None, 'channel', 'fzyx'),
}
# (dtype, zero_centered) of every lattice above: what the plain pins do not cover
VARIANTS = [('float16', False), ('float16', True), ('float32', True), ('float64', True)]


def kernels(name, dtype, zero_centered, target):
    """The ``LatticeKernels`` of lattice ``name`` for ``dtype`` pdfs on ``target`` ('gpu' / 'cpu')."""
    stencil, shape, method, compressible, fm, walls, layout = LATTICES[name]
    D = len(shape)
    kw = {}
    if method == 'trt':
        kw = dict(method='trt')
    elif method == 'mrt':
        kw = dict(method='mrt', relaxation_rates=[sp.Symbol('omega'), 1.1, 0.9, 1.2])
    if fm:
        kw.update(force_model=fm, force=(1e-3, -2e-3, 5e-4)[:D])
    rule = lbm.create_lb_update_rule(stencil, compressible=compressible, data_type=dtype, layout=layout,
                                     zero_centered=zero_centered, **kw)
    step = lbm.AutoDiffLatticeBoltzmannStep(rule, domain_size=shape, relaxation_rate=1.3, target=target)
    if walls == 'channel':
        step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, 0])
        step.set_boundary_including_adjoint(lbm.NoSlip(), lbm.make_slice[:, -1])
    elif walls == 'cavity':
        for sl in (lbm.make_slice[0, :], lbm.make_slice[-1, :], lbm.make_slice[:, 0]):
            step.set_boundary_including_adjoint(lbm.NoSlip(), sl)
        step.set_boundary_including_adjoint(lbm.UBB((0.05,) + (0.0,) * (D - 1), name='lid'), lbm.make_slice[1:-1, -1])
    assert step._lattice is not None
    return step._lattice_kernels()


def shas():
    def sha(s):
        return hashlib.sha256(s.encode()).hexdigest()
    out = {}
    for name in LATTICES:
        for dtype, zc in VARIANTS:
            key = f'{name}/{dtype}{"-zc" if zc else ""}'
            out[f'{key}/c'] = sha(kernels(name, dtype, zc, 'cpu').source())
            K = kernels(name, dtype, zc, 'gpu')
            for idx in ('int', 'long long'):
                for addr in ('buf', 'ptr'):
                    out[f'{key}/hip-{idx.replace(" ", "")}-{addr}'] = sha(K.source(idx, addr))
    return out


if __name__ == '__main__':
    table = shas()
    with open(PATH, 'w') as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write('\n')
    print(f'{len(table)} sources -> {PATH}')
