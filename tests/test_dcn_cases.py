"""The builders of tests/dcn_cases.py keep their promises (CPU): the positions are where they are meant to be, and the oracle's
gradient at the taps that sit exactly on a clamp bound is non-zero and large -- so a kernel whose clamp gate were strict would
fail tests/test_gpu_dcn_edges.py at the tensor level, not only in the zero pattern."""
import pytest
import torch

import dcn_cases as dc


def _off_grads(name):
    c = dc.get(name)
    N, H, W, C, K, stride = c['shape']
    Ho, Wo = dc.out_hw(H, W, stride)
    dom = dc.oracle(name)['dom']
    d = dom[:, :18].permute(0, 2, 3, 1).reshape(N, Ho, Wo, 9, 2)
    return c, dom, d[..., 0], d[..., 1]


@pytest.mark.parametrize('name', [n for n in dc.CASES if n.startswith('zero')])
def test_zero_offsets_sit_on_both_clamp_bounds(name):
    c, dom, dyo, dxo = _off_grads(name)
    N, H, W, C, K, stride = c['shape']
    assert not c['om'][:, :18].any()
    assert not c['om'][:, 18:].any() or name.endswith('random')
    py, px, ymax, xmax = dc.positions(c)
    assert torch.equal(py, py.floor()) and torch.equal(px, px.floor())            # lh = lw = 0 everywhere
    assert (py == 0).any() and (px == 0).any()                                    # ho = 0, kh = 0
    assert ((py == ymax).any() and (px == xmax).any()) == (stride == 1)           # last row, kh = 2
    # ON the lower bound the sample blends the padding row with image row 0: d / d offset = the mask-weighted image row, non-zero;
    # torch.clamp passes it.  ON the upper bound H+2p-1 both rows of the blend lie in the padding: the gradient is 0 whatever the gate.
    lo_y, lo_x = (py == 0) & (px >= 1) & (px <= W), (px == 0) & (py >= 1) & (py <= H)
    assert lo_y.sum() >= N * 3 and (dyo[lo_y] != 0).all() and (dxo[lo_x] != 0).all()
    assert not dyo[py == ymax].any() and not dxo[px == xmax].any()
    mx = dom.abs().max()
    assert dyo[lo_y].abs().max() >= 1e-2 * mx and dxo[lo_x].abs().max() >= 1e-2 * mx
    assert torch.isfinite(dom).all()


@pytest.mark.parametrize('name', [n for n in dc.CASES if n.startswith('exact')])
def test_exact_positions_cover_every_kind(name):
    c, dom, dyo, dxo = _off_grads(name)
    N, H, W, C, K, stride = c['shape']
    py, px, ymax, xmax = dc.positions(c)
    kinds = c['kinds']
    for d, (p, mx, grad) in enumerate(((py, ymax, dyo), (px, xmax, dxo))):
        k = kinds[..., d]
        assert all((k == i).sum() >= 5 for i in range(len(dc.KINDS)))
        assert torch.equal(p * 2, (p * 2).floor())                                # integers and half-integers, exactly
        assert (p[k == 4] == 0).all() and (p[k == 5] == mx).all() and (p[k == 6] == -1).all() and (p[k == 7] == mx + 1).all()
        assert ((p[k == 2] % 1) == 0.5).all()
        assert not grad[(p < 0) | (p > mx)].any()                                 # beyond a bound: gate 0, exactly 0
        assert (grad[k == 4] != 0).sum() >= 3                                     # on the bound (through an offset): passed
    assert (dyo[(py >= 0) & (py <= ymax)] != 0).sum() > (dyo != 0).sum() * 0.99


def test_collisions_land_on_four_pixels():
    name = [n for n in dc.CASES if n.startswith('collide')][0]
    c = dc.get(name)
    py, px, ymax, xmax = dc.positions(c)
    assert (py - py[0, 0, 0, 0]).abs().max() <= 1e-6 and (px - px[0, 0, 0, 0]).abs().max() <= 1e-6
    assert 0 < py[0, 0, 0, 0] % 1 < 1 and 0 < px[0, 0, 0, 0] % 1 < 1
    dx = dc.oracle(name, torch.float64)['dx']
    assert int(dx.abs().amax(dim=(0, 1)).gt(0).sum()) == 4


@pytest.mark.parametrize('name', sorted(dc.CASES))
def test_float32_and_float64_oracles_agree(name):
    a, b = dc.oracle(name, torch.float32), dc.oracle(name, torch.float64)
    for k in ('dx', 'dom', 'dw'):
        assert torch.isfinite(a[k]).all()
        assert (a[k].double() - b[k]).abs().max() <= 2e-5 * b[k].abs().max(), (name, k)
    d32, d64 = a['dom'][:, :18], b['dom'][:, :18]
    assert torch.equal(d32 == 0, d64 == 0)


def test_layout_cases_reach_the_channel_loops():
    cs = sorted(dc.get(n)['shape'][3] for n in dc.CASES if n.startswith('layout'))
    assert cs == [96, 320] and 96 % 64 != 0 and 320 > 256
