"""Host side of ``ops`` that needs no device: the layer's reversed block layout, and the one
preparation of ``y_mean`` / ``y_std`` every entry point goes through."""

import numpy as np
import pytest
import torch

from normalizingflownetwork_amd import ops
from oracle import nfn_oracle as O


@pytest.mark.parametrize("ft,d,tb", [(("planar", "radial"), 1, True), (("planar", "radial", "affine"), 3, False),
                                     (("affine", "planar", "radial"), 8, True)])
def test_flow_block_offsets_equal_the_oracle_split(ft, d, tb):
    """Flow k's block starts where the oracle's own split of a row of column numbers puts it
    (``DistributionLayers.py:267-278``: blocks in REVERSED flow order after the base's 2 d)."""
    P = O.total_param_size(ft, d, tb)
    _, blocks = O.split_params(np.arange(P)[None, :], ft, d, tb)
    offs = ops.flow_block_offsets(ft, d, tb)
    assert list(offs) == [int(b[0, 0]) for b in blocks]
    assert [len(b[0]) for b in blocks] == [ops.param_size(f, d) for f in ft]
    assert max(o + ops.param_size(f, d) for o, f in zip(offs, ft)) == P == ops.total_param_size(ft, d, tb)


def test_norm_stats_checks_both_lengths():
    """The kernels read ``n_dims`` floats of ``y_mean`` and of ``y_std``: a short array is
    refused on the host, by the one helper every entry point prepares them with."""
    cpu = torch.device("cpu")
    assert ops._norm_stats(None, None, 3, cpu) == (None, None)
    ym, ys = ops._norm_stats([0.0, 1.0, 2.0], np.array([[1.0], [2.0], [3.0]]), 3, cpu)
    assert ym.shape == ys.shape == (3,) and ym.dtype == ys.dtype == torch.float32 and ys.is_contiguous()
    assert ys.tolist() == [1.0, 2.0, 3.0]
    assert ops._norm_stats(0.5, 2.0, 1, cpu)[1].tolist() == [2.0]
    with pytest.raises(AssertionError):
        ops._norm_stats([0.0, 1.0, 2.0], [1.0, 2.0], 3, cpu)
    with pytest.raises(AssertionError):
        ops._norm_stats([0.0, 1.0], [1.0, 2.0, 3.0], 3, cpu)
