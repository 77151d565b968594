"""Plain float64 restatements of the four kernels of csrc/pool_tokens.hip -- svl_gap_tokens_fwd / _bwd, svl_bcast_rows_fwd /
_bwd -- each from the header's index formula (include/semivl_hip.h), none from the kernels and none from the tensor
expressions they stand for (tests/test_pool_tokens_ref.py proves them against `x.view(b, HW, C).mean(1)`, its autograd,
`expand` and `sum`).  Device-agnostic; the guard-band helpers, gamma() and the unit roundoff come from tests/spatial_ref.py.

Bounds (Higham, lemma 3.1, as in tests/spatial_ref.py): the sums are accumulated in double and rounded to fp32 once, so
the longest fp32 chain of the two sum kernels is ONE operation: |error| <= gamma(1) * sum |terms| (the double accumulation
itself adds HW * 2^-53 relative to the same sum of absolute terms -- below gamma(1) - u for every HW < 2^28).  The mean's
division happens in double before that rounding.  svl_gap_tokens_bwd divides two fp32 numbers, correctly rounded: one
operation; its accumulating form adds the base: two.  The broadcast copies: equal bits."""
import torch

from spatial_ref import AGUARD, SENTINEL, U, gamma, gaps_intact, one_pass, strided  # noqa: F401  (re-exported for the test files)

GAP_CH = 64                      # channels one block of the column-sum kernel owns (csrc/pool_tokens.hip)
GRID_CAP = 256 * 32              # blocks either kernel family launches at most


def _img_of_row(imgs, HW, device):
    return torch.arange(imgs * HW, dtype=torch.int64, device=device) // HW


def gap_fwd_ref(x, imgs, HW, mean=True):
    """(want, bound) float64 [imgs, C]: pool[img, c] = (1 / HW) sum_p x[img * HW + p, c]  (mean=False: the plain sum,
    svl_bcast_rows_bwd).  Row by row with index_add_ on the header's row index."""
    xd = x.double()
    idx = _img_of_row(imgs, HW, x.device)
    want = torch.zeros(imgs, x.shape[1], dtype=torch.float64, device=x.device).index_add_(0, idx, xd)
    mag = torch.zeros_like(want).index_add_(0, idx, xd.abs())
    if mean:
        want, mag = want / HW, mag / HW
    return want, gamma(1) * mag


def gap_bwd_ref(dpool, imgs, HW, base=None):
    """(want, bound) float64 [imgs * HW, C]: dx[img * HW + p, c] = dpool[img, c] / HW (+ base)."""
    t = dpool.double().index_select(0, _img_of_row(imgs, HW, dpool.device)) / HW
    if base is None:
        return t, gamma(1) * t.abs()
    return base.double() + t, gamma(2) * (base.double().abs() + t.abs())


def bcast_fwd_ref(v, imgs, HW):
    """fp32 [imgs * HW, C]: row img * HW + p holds v[img] (a copy: compared for equality)."""
    return v.index_select(0, _img_of_row(imgs, HW, v.device))


def bcast_bwd_ref(dy, imgs, HW):
    """(want, bound) float64 [imgs, C]: dv[img, c] = sum_p dy[img * HW + p, c]."""
    return gap_fwd_ref(dy, imgs, HW, mean=False)


# ---------------------------------------------------------------------------------------------------------------- cases
# (imgs, HW, C): one image and several; one pixel (the sum is the term), a few, and more rows than a block's row lanes
# visit once (16 lanes x 30 rows); C below a quad, one full 64-channel group, and three groups with a ragged last one.
CASES = [(imgs, HW, C) for imgs in (1, 3) for HW in (1, 7, 480) for C in (3, 64, 130)]
# (name, row-stride slack, channel offset): 16-byte paths where C % 4 == 0, and an odd offset in an odd stride (scalar)
LAYOUTS = [("aligned", 8, 4), ("odd", 7, 3)]
BIG_ELTWISE = (2, 16400, 256)    # 2 * 16400 * 64 quads > 256 * 32 * 256: the broadcast / gradient kernels loop
BIG_SUM = (4100, 2, 130)         # 4100 images x 3 channel groups > 256 * 32 blocks: the sum kernel loops


def inputs(case, seed=0):
    """x [imgs * HW, C], dpool [imgs, C], base [imgs * HW, C] (fp32, seeded; values of mixed sign and magnitude)."""
    imgs, HW, C = case
    g = torch.Generator().manual_seed(1000 * imgs + 10 * HW + C + seed)
    x = torch.randn(imgs * HW, C, generator=g) * (1.0 + 3.0 * torch.rand(1, C, generator=g))
    dpool = torch.randn(imgs, C, generator=g)
    base = torch.randn(imgs * HW, C, generator=g)
    return x, dpool, base
