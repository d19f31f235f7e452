"""The backward restatement (tests/backward_restate.py) tested on the CPU, before the GPU tests lean on it: against torch
autograd through the oracle's convolution on the maps of a batched pair of fixture fragments, the opposite-map identities
imfnet_amd/autograd.py relies on, the inner-product identity, the synthetic-map builder, and the fp32 headroom of the
integer data on the largest geometry tests/test_gpu_backward_exact.py uses."""
import numpy as np
import pytest
import torch

import backward_restate as R
import imf_oracle as O

# (transposed, kernel_size, stride, tensor stride of the input, cin, cout): every kind of map, at every level it occurs
KINDS = [(False, 5, 1, 1, 1, 8), (False, 3, 1, 1, 8, 8), (False, 3, 1, 2, 8, 4), (False, 3, 1, 4, 4, 8),
         (False, 3, 1, 8, 8, 8), (False, 3, 2, 1, 8, 4), (False, 3, 2, 2, 4, 8), (False, 3, 2, 4, 8, 8),
         (True, 3, 2, 8, 8, 4), (True, 3, 2, 4, 12, 8), (True, 3, 2, 2, 8, 8), (False, 1, 1, 1, 12, 8)]


@pytest.fixture(scope="module")
def geo(clouds):
    _, coords = R.batched_voxels([clouds[0][::2], clouds[1][::2]], 0.05)
    assert set(coords[:, 0].tolist()) == {0, 1}
    return O.Geometry(coords)


def _case(geo, sig, seed):
    tr, ks, st, ts, cin, cout = sig
    nbr, kind, lv, n_in, n_out = R.layer_map(geo, tr, ks, st, ts)
    feat, W, g = R.int_case(torch.Generator().manual_seed(seed), n_in, n_out, ks ** 3, cin, cout)
    return nbr, kind, lv, feat, W, g


@pytest.mark.parametrize("sig", KINDS, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_restatement_equals_torch_autograd_through_the_oracle(geo, sig):
    nbr, kind, lv, feat, W, g = _case(geo, sig, 11)
    out, dX, dW = R.conv_restate(feat, W, g, nbr)
    f = feat.clone().requires_grad_(True)
    w = (W[0] if kind == "k1" else W).clone().requires_grad_(True)
    ref = O.spconv(f, w, nbr)
    ref.backward(g)
    assert ref.dtype == torch.float32
    assert torch.equal(out, ref.detach().double())
    assert torch.equal(dX, f.grad.double())
    assert torch.equal(dW, w.grad.double().reshape(dW.shape))
    assert float(dW.abs().max()) > 0 and float(dX.abs().max()) > 0
    # the float64 oracle agrees too (the yardstick of the float cases)
    assert torch.equal(out, O.spconv_f64(feat, W[0] if kind == "k1" else W, nbr))
    # <conv(x), g> = <x, dX> = <W, dW>, as integers
    a, b, c = R.inner_products(feat, W, g, out, dX, dW)
    assert a == b == c and a != 0


@pytest.mark.parametrize("sig", [s for s in KINDS if s[1] > 1], ids=lambda s: "-".join(str(int(v)) for v in s))
def test_input_gradient_is_the_convolution_over_the_opposite_map(geo, sig):
    nbr, kind, lv, feat, W, g = _case(geo, sig, 12)
    _, dX, _ = R.conv_restate(feat, W, g, nbr)
    Wt, nbr_t = R.opposite(W, kind, geo, lv)
    assert nbr_t.shape[0] == feat.shape[0]
    assert torch.equal(dX, R.conv_restate(g, Wt, None, nbr_t))
    assert torch.equal(dX.float(), O.spconv(g, Wt.contiguous(), nbr_t))
    if kind in ("k3", "k5"):                       # without the flip the identity must NOT hold (the test can fail)
        assert not torch.equal(dX, R.conv_restate(g, W.transpose(1, 2), None, nbr_t))


def test_synthetic_maps_round_trip():
    gen = torch.Generator().manual_seed(5)
    for n_out, n_slots, permute, empty in ((1, None, False, ()), (65, None, True, (0, 26)), (4096, 8192, True, (13,)),
                                           (4097, None, False, ()), (300, 4096, True, ())):
        rows, tile_rows, tiled = R.synthetic_map(gen, n_out, 77, 27, n_slots=n_slots, permute=permute, empty_offsets=empty)
        n_s = len(tile_rows)
        assert n_s % 64 == 0 and n_s >= n_out and tiled.shape == (27, n_s) and rows.shape == (n_out, 27)
        assert int((tile_rows < 0).sum()) == n_s - n_out and (tiled[:, tile_rows < 0] == -1).all()
        assert rows.max() < 77 and rows.min() >= -1 and all((rows[:, k] == -1).all() for k in empty)
        assert np.array_equal(R.tiled_to_rows(tile_rows, tiled, n_out), rows)
        tr2, tiled2 = R.rows_to_tiled(rows, n_s, tile_rows)
        assert np.array_equal(tr2, tile_rows) and np.array_equal(tiled2, tiled)
        if permute and n_out > 64:
            assert not np.array_equal(tile_rows[:n_out], np.arange(n_out))
        else:
            assert np.array_equal(R.tiled_to_rows(None, tiled, n_out), rows)      # identity order: tile_rows may be NULL
    # a map that loses a row is refused
    rows, tile_rows, tiled = R.synthetic_map(gen, 100, 50, 27)
    bad = tile_rows.copy()
    bad[3] = 4
    with pytest.raises(AssertionError):
        R.tiled_to_rows(bad, tiled, 100)
    # the restatement over the round-tripped map is the restatement over the rows: dW by hand for one offset
    feat, W, g = R.int_case(gen, 50, 100, 27, 3, 5)
    _, _, dW = R.conv_restate(feat, W, g, rows, n_in=50)
    k = 7
    want = torch.zeros(3, 5, dtype=torch.float64)
    for o in range(100):
        if rows[o, k] >= 0:
            want += torch.outer(feat[rows[o, k]].double(), g[o].double())
    assert torch.equal(dW[k], want)


def test_integer_data_stays_exact_in_fp32_on_the_largest_geometry(clouds):
    """The largest maps of the GPU file: one whole fixture fragment at 2.5 cm and the batch of both at 5 cm, at the
    network's widest layers (256 channels, 192 into a transposed convolution), and the 40 000-row synthetic map."""
    for point_sets, voxel in (([clouds[0]], 0.025), ([clouds[0], clouds[1]], 0.05)):
        _, coords = R.batched_voxels(point_sets, voxel)
        g = O.Geometry(coords)
        n = [len(c) for c in g.levels]
        if voxel == 0.025:
            assert n[0] > 3 * 4096                      # the level-0 weight gradient spans at least four chunks
        for nbr, n_in in [(g.k_first, n[0])] + [(g.k3[i], n[i]) for i in range(4)] + \
                [(g.down[i], n[i]) for i in range(3)] + [(g.up[i], n[i + 1]) for i in range(3)]:
            assert max(R.magnitude_bounds(nbr, n_in, 256, 256)) < R.EXACT_LIMIT
        assert max(R.magnitude_bounds(None, n[0], 256, 256)) < R.EXACT_LIMIT
    rows, _, _ = R.synthetic_map(torch.Generator().manual_seed(1), 40000, 40000, 27, density=0.5)
    assert max(R.magnitude_bounds(rows, 40000, 256, 256)) < R.EXACT_LIMIT
    assert max(R.magnitude_bounds(None, 40000, 256, 256)) < R.EXACT_LIMIT
    # the bound is a bound: measured magnitudes on a real case stay under it
    _, coords = R.batched_voxels([clouds[0][::2], clouds[1][::2]], 0.05)
    g = O.Geometry(coords)
    feat, W, go = R.int_case(torch.Generator().manual_seed(2), len(g.levels[1]), len(g.levels[1]), 27, 16, 16)
    out, dX, dW = R.conv_restate(feat, W, go, g.k3[1])
    b = R.magnitude_bounds(g.k3[1], len(g.levels[1]), 16, 16)
    for got, bound in zip((out, dX, dW), b):
        assert 0 < float(got.abs().max()) <= bound
