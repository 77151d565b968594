"""GpuAugmenter(unlabeled_gt=True): the unlabelled samples' annotation comes through the image's own geometry as `mask_u`;
without the flag the batch keeps its 12 keys."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KEYS12 = {"img_x", "mask_x", "img_w", "img_s1", "img_s2", "ignore_mask", "mix1", "mix2", "img_w_other", "img_s1_other",
          "img_s2_other", "ignore_mask_other"}


def _sample(seed, h=100, w=140):
    rng = np.random.RandomState(seed)
    mask = np.repeat(np.repeat(rng.randint(0, 21, (h // 10, w // 10)), 10, 0), 10, 1).astype(np.uint8)
    mask[rng.rand(h, w) < 0.03] = 255                                  # void
    return torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)), torch.from_numpy(mask)


def test_mask_u_is_the_mask_through_the_recorded_draw(dev, monkeypatch):
    from semivl_amd import data
    random.seed(3); np.random.seed(3)
    S, B = 64, 3
    calls = []
    real = data.resample

    def recording(src, rh, rw, x0, y0, S_, flip, nearest=False, fill=0, cv2=False):
        out = real(src, rh, rw, x0, y0, S_, flip, nearest=nearest, fill=fill, cv2=cv2)
        if nearest:
            calls.append((src.clone(), (rh, rw, x0, y0, S_, flip), fill, cv2))
        return out

    monkeypatch.setattr(data, "resample", recording)
    aug = data.GpuAugmenter(S, (0.5, 2.0), device=dev, unlabeled_gt=True)
    # (the last unlabelled sample is 30 x 40: at most 60 x 80 after the resize, so the 64-crop always pads it)
    lab, unl = [_sample(i) for i in range(B)], [_sample(10, 100, 140), _sample(11, 120, 90), _sample(12, 30, 40)]
    batch = aug.batch(lab, unl, unl)
    monkeypatch.setattr(data, "resample", real)
    assert set(batch) == KEYS12 | {"mask_u"}
    mu = batch["mask_u"]
    assert mu.dtype == torch.int64 and mu.shape == batch["ignore_mask"].shape == (B, S, S) and mu.is_contiguous()
    # draws: B labelled masks, then the B unlabelled samples of the first view, then the "other" view's
    assert len(calls) == 3 * B
    for i in range(B):
        src, draw, fill, cv2 = calls[B + i]
        assert fill == 254 and torch.equal(src.cpu(), unl[i][1])
        want = real(unl[i][1].to(dev), *draw, nearest=True, fill=254, cv2=cv2)
        assert torch.equal(mu[i], want.to(torch.int64))
    # 254 exactly on the padding, void (255) and the classes left as they are
    assert torch.equal(mu == 254, batch["ignore_mask"] == 255)
    assert (batch["ignore_mask"][2] == 255).any()
    vals = set(mu.unique().tolist())
    assert vals <= set(range(21)) | {254, 255} and 255 in vals and len(vals & set(range(21))) > 1


def test_default_keeps_the_twelve_keys(dev):
    from semivl_amd import data
    random.seed(4); np.random.seed(4)
    aug = data.GpuAugmenter(64, (0.5, 2.0), device=dev)
    assert aug.unlabeled_gt is False
    unl = [_sample(30), _sample(31)]
    batch = aug.batch([_sample(1), _sample(2)], unl, unl)
    assert set(batch) == KEYS12
    assert len(aug.train_u(*unl[0])) == 6
    assert len(data.GpuAugmenter(64, device=dev, unlabeled_gt=True).train_u(*unl[0])) == 7
