"""What the four GPU suites of the plane-streaming kernels (test_score_gpu, test_ensemble_gpu, test_quantile_gpu, test_dataset_stats_gpu)
share: the device and library fixtures (imported by name into each of them), sentinel-guarded device buffers and the row weights."""
import numpy as np
import pytest
import torch

SENTINEL = 0x7FC0BEEF          # as int32: a NaN payload no kernel produces; two of them make an fp64 NaN no kernel produces either
GUARD = 64                     # int32 words in front of and behind every buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from swin_v2_weather_amd import _lib as L
    return L.load()                                  # fails loudly if libswv2.so is missing: no fallback exists


def _weights(H):
    from swin_v2_weather_amd.utils.weighted_acc_rmse import latitude_weights
    return latitude_weights(H).numpy() if H > 1 else np.ones(1, np.float32)          # (the formula divides by H - 1)


class Guarded:
    """device buffers carved out of one int32 allocation filled with `fill`, each 16-byte aligned with GUARD words on both sides.
    A buffer is given as its element count, of `dtype` unless it is a (count, dtype) pair: torch.float32, torch.int32 or torch.float64."""

    def __init__(self, dev, fill=SENTINEL, dtype=torch.float32, **sizes):
        self.off, n = {}, GUARD
        for k, v in sizes.items():
            count, dt = v if isinstance(v, tuple) else (v, dtype)
            words = count * (2 if dt == torch.float64 else 1)
            self.off[k] = (n, words, dt)
            n += (words + 3) // 4 * 4 + GUARD
        self.raw = torch.full((n,), fill, dtype=torch.int32, device=dev)
        self.fill, self.sizes = fill, sizes
        assert self.raw.data_ptr() % 16 == 0

    def ints(self, k):
        o, words, _ = self.off[k]
        return self.raw[o:o + words]

    def __getitem__(self, k):
        return self.ints(k).view(self.off[k][2])

    def guards_intact(self):
        keep = torch.ones(self.raw.numel(), dtype=torch.bool, device=self.raw.device)
        for o, words, _ in self.off.values():
            keep[o:o + words] = False
        return bool((self.raw[keep] == self.fill).all())

    def written(self, k):
        return bool((self.ints(k) != SENTINEL).all())
