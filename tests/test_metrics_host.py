"""Host half of the device scoring path (no GPU): the PSNR formula applied to the kernel's exact integer sums, the
argument check of validate_batch, and the new C-ABI symbol in the header and the ctypes table."""
import math
import os

import numpy as np
import pytest

from conftest import REPO, pkg

metrics = pkg("metrics")
validation = pkg("validation")


def _pairs(side):
    rs = np.random.RandomState(1000 + side)
    shape = (side, side, 3)
    a = rs.randint(0, 256, shape).astype(np.uint8)
    yield "noise", a, rs.randint(0, 256, shape).astype(np.uint8)
    yield "close", a, np.clip(a.astype(np.int64) + rs.randint(-2, 3, shape), 0, 255).astype(np.uint8)
    yield "one pixel", a, np.where(np.arange(a.size).reshape(shape) == 7, a ^ 1, a).astype(np.uint8)
    yield "identical", a, a.copy()
    yield "255 vs 0", np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)


@pytest.mark.parametrize("side", [16, 128])
def test_scores_from_sums_is_bit_equal_to_host_psnr(side):
    names, ssd, want = [], [], []
    for name, a, b in _pairs(side):
        d = a.astype(np.int64) - b.astype(np.int64)
        names.append(name)
        ssd.append(int((d * d).sum()))
        want.append(metrics.psnr(a, b))
    got = validation.scores_from_sums(np.array(ssd, dtype=np.int64), 3 * side * side)
    assert got.dtype == np.float64 and got.shape == (len(ssd),)
    for name, g, w in zip(names, got, want):
        assert g == w and (math.isinf(w) or g.tobytes() == np.float64(w).tobytes()), (name, g, w)
    assert math.isinf(got[names.index("identical")]) and got[names.index("identical")] > 0
    assert got[names.index("255 vs 0")] == 0.0
    # shape is kept, sums beyond 32 bits are taken as they are
    big = validation.scores_from_sums(np.array([[3 * 224 * 224 * 65025, 1]], dtype=np.int64), 3 * 224 * 224)
    assert big.shape == (1, 2) and big[0, 0] == 0.0 and big[0, 1] == 20 * math.log10(255.0 / math.sqrt(1.0 / (3 * 224 * 224)))


def test_validate_batch_rejects_unknown_metrics_before_any_gpu_work():
    # neither the network nor the tensors are touched: the check comes first
    with pytest.raises(ValueError, match="metrics"):
        validation.validate_batch(None, None, None, samples=2, metrics="gpu")
    with pytest.raises(ValueError, match="metrics"):
        validation.validate_batch(None, None, None, metrics=None)


def test_metrics_symbol_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "sr3hip.h")).read()
    assert "int sr3_metrics_psnr_ssim(sr3_ctx *ctx, const float *sr_nchw_dev, const float *hr_nchw_dev" in header
    protos = pkg("_lib").PROTOTYPES
    assert "sr3_metrics_psnr_ssim" in protos
    res, args = protos["sr3_metrics_psnr_ssim"]
    assert len(args) == 11          # ctx, sr, hr, B, N, row_offset, H, W, taps, ssd, ssim
    assert "kernels_metrics.hip" in pkg("build").SOURCES
