"""Z-slabs of ``boundary_handling='periodic'`` kernels: the exchange wraps around (every rank has two neighbours; with
two ranks both are the same rank and the faces go out swapped), x and y wrap inside the kernels. The workers, the gloo
stand-in for the RCCL exchange and the port helper are ``tests/test_distributed.py``'s; the reference is the fully
periodic one of ``tests/test_periodic_march.py`` (wrap-padded inputs through the float64 oracle) — ``_run``'s own
reference is the 'zeros' one and is ignored. Only the gloo emulation and the loopback communicator exercise the exchange
code here: no multi-rank RCCL run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests.test_distributed import ROOT, _dtype, _run  # noqa: E402
from tests.test_periodic_march import periodic_reference  # noqa: E402


def _reference(builder_name, shape, seed=0):
    """(u, d, out, diffu): ``_worker``'s inputs (its seed and draw order) and the periodic forward / adjoint."""
    import sys
    sys.path.insert(0, ROOT)
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import workloads as W
    op = pa.AutoDiffOp(getattr(W, builder_name)(), boundary_handling='periodic')
    rng = np.random.default_rng(seed)
    dt = _dtype(builder_name)
    u = rng.uniform(0, 1, shape).astype(dt)
    d = rng.uniform(-1, 1, shape).astype(dt)
    out = periodic_reference(op.forward_assignments, {'u': u}, 1)['out']
    du = periodic_reference(op.backward_assignments, {'diffout': d}, 1)['diffu']
    return u, d, out, du


def _assert(builder_name, shape, out, du):
    from tests.conftest import assert_close_rel
    _, _, ref_out, ref_du = _reference(builder_name, shape)
    tol = 1e-3 if _dtype(builder_name) == np.float16 else 1e-6
    assert_close_rel(out, ref_out, tol, 'out')
    assert_close_rel(du, ref_du, tol, 'diffu')


# ---------------------------------------------------------------------------------------------------------- CPU, gloo
@pytest.mark.parametrize('world,shape', [(2, (10, 9, 12)), (3, (13, 6, 7))])
@pytest.mark.parametrize('builder_name', ['asym_7pt', 'diffusion_7pt'])
def test_zslab_periodic_gloo_cpu(world, shape, builder_name, tmp_path):
    """Two ranks: both neighbours are one rank (a missing face swap exchanges the halos); three: a wrap-around pair."""
    out, du, _, _ = _run(world, shape, builder_name, False, tmp_path, bh='periodic')
    _assert(builder_name, shape, out, du)


def test_zslab_periodic_autograd_function_gloo_cpu(tmp_path, monkeypatch):
    monkeypatch.setenv('PSAD_TEST_ZSLAB_AUTOGRAD', '1')
    out, du, _, _ = _run(2, (11, 8, 9), 'asym_7pt', False, tmp_path, bh='periodic')
    _assert('asym_7pt', (11, 8, 9), out, du)


def test_periodic_neighbours_and_face_swap():
    """Peers wrap for periodic kernels only; the faces swap exactly where both peers are one rank."""
    import sys
    sys.path.insert(0, ROOT)
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import workloads as W
    from pystencils_autodiff_amd.zslab import ZSlabOp

    class Halo:
        def __init__(self, rank, world, loopback=False):
            self.rank, self.world, self.loopback = rank, world, loopback
    per = ZSlabOp(pa.AutoDiffOp(W.asym_7pt(), boundary_handling='periodic'), use_cuda=False)
    zer = ZSlabOp(pa.AutoDiffOp(W.asym_7pt(), boundary_handling='zeros'), use_cuda=False)
    assert [per._peers(Halo(r, 3)) for r in range(3)] == [(2, 1), (0, 2), (1, 0)]
    assert [per._peers(Halo(r, 2)) for r in range(2)] == [(1, 1), (0, 0)]
    assert [zer._peers(Halo(r, 3)) for r in range(3)] == [(-1, 1), (0, 2), (1, -1)]
    assert [per._swap_faces(Halo(r, 2)) for r in range(2)] == [True, True]
    assert not any(per._swap_faces(Halo(r, 3)) for r in range(3))
    assert not any(zer._swap_faces(Halo(r, 2)) for r in range(2))
    assert per._swap_faces(Halo(0, 1, loopback=True)) and zer._swap_faces(Halo(0, 1, loopback=True))
    assert per.z_limits(per.kernels['forward'], 5) == (0, 5)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _gpu_inputs(builder_name, shape, seed):
    u, d, ref_out, ref_du = _reference(builder_name, shape, seed)
    return torch.from_numpy(u).cuda(), torch.from_numpy(d).cuda(), ref_out, ref_du


@pytest.mark.gpu
def test_zslab_periodic_one_rank_without_a_communicator():
    """No exchange and no halos: the kernel wraps z itself."""
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import workloads as W
    from pystencils_autodiff_amd.zslab import ZSlabOp
    from tests.conftest import assert_close_rel
    shape = (12, 40, 64)
    z = ZSlabOp(pa.AutoDiffOp(W.asym_7pt(), boundary_handling='periodic'), use_cuda=True)
    tu, td, ref_out, ref_du = _gpu_inputs('asym_7pt', shape, 5)
    out, du = torch.empty_like(tu), torch.empty_like(td)
    z.fwd(u=tu, out=out)
    z.bwd(diffout=td, diffu=du)
    torch.cuda.synchronize()
    assert z.kernels['forward'].compile().last_variant[0] == 'march'
    assert_close_rel(out.cpu().numpy(), ref_out, 1e-6, 'out')
    assert_close_rel(du.cpu().numpy(), ref_du, 1e-6, 'diffu')


@pytest.mark.gpu
@pytest.mark.parametrize('builder_name,shape,native', [('asym_7pt', (12, 40, 72), True),
                                                       ('stencil_27pt', (9, 24, 80), True),
                                                       ('diffusion_7pt', (2, 9, 64), False),
                                                       ('diffusion_7pt', (3, 17, 64), False)])
def test_zslab_periodic_rccl_loopback(builder_name, shape, native, monkeypatch):
    """The loopback communicator's exchange is a periodic-z exchange: with periodic kernels the RCCL sweep
    (``_sweep_rccl``) and the native slab node give the FULLY periodic stencil."""
    import pystencils_autodiff_amd as pa
    from pystencils_autodiff_amd import workloads as W
    from pystencils_autodiff_amd.zslab import RcclHalo, ZSlabOp
    from tests.conftest import assert_close_rel
    op = pa.AutoDiffOp(getattr(W, builder_name)(), boundary_handling='periodic')
    tol = 1e-3 if _dtype(builder_name) == np.float16 else 1e-6
    tu, td, ref_out, ref_du = _gpu_inputs(builder_name, shape, 5)
    z = ZSlabOp(op, use_cuda=True)
    z._halo = RcclHalo(loopback=True)
    try:
        out, du = torch.empty_like(tu), torch.empty_like(td)
        z.warm_exchange(u=tu, diffout=td)
        for which, kw in (('forward', dict(u=tu, out=out)), ('backward', dict(diffout=td, diffu=du))):
            k = z.kernels[which]
            z._sweep_rccl(k, z._halo, k.ir.stencil_fields, 1, kw)
        torch.cuda.synchronize()
        assert z.kernels['forward'].compile().last_variant[0] == 'march'
        assert_close_rel(out.cpu().numpy().astype(np.float64), ref_out, tol, 'out')
        assert_close_rel(du.cpu().numpy().astype(np.float64), ref_du, tol, 'diffu')
        if native:
            monkeypatch.setenv('PSAD_NATIVE_SLAB', '1')
            fn = z.autograd_function()
            uu = tu.clone().requires_grad_(True)
            (o,) = fn.apply(uu)
            assert 'CppNode' in o.grad_fn.name(), o.grad_fn.name()
            o.backward(td)
            torch.cuda.synchronize()
            assert_close_rel(o.detach().cpu().numpy().astype(np.float64), ref_out, tol, 'native out')
            assert_close_rel(uu.grad.cpu().numpy().astype(np.float64), ref_du, tol, 'native diffu')
    finally:
        z.close()


@pytest.mark.gpu
@pytest.mark.parametrize('world,shape', [(2, (24, 40, 64)), (3, (19, 33, 72))])
@pytest.mark.parametrize('builder_name', ['asym_7pt', 'stencil_27pt'])
def test_zslab_periodic_rccl_sweep_emulated_ranks(world, shape, builder_name, tmp_path, monkeypatch):
    monkeypatch.setenv('PSAD_TEST_EMULATED_RCCL', '1')
    out, du, _, _ = _run(world, shape, builder_name, True, tmp_path, bh='periodic')
    _assert(builder_name, shape, out, du)


@pytest.mark.gpu
@pytest.mark.parametrize('builder_name', ['asym_7pt', 'diffusion_7pt'])
def test_zslab_periodic_gloo_gpu_halo_path(builder_name, tmp_path):
    assert not os.environ.get('PSAD_TEST_EMULATED_RCCL')
    out, du, _, _ = _run(2, (24, 40, 64), builder_name, True, tmp_path, bh='periodic')
    _assert(builder_name, (24, 40, 64), out, du)
