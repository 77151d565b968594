"""svl_pl_stats_i64's table (include/semivl_hip.h) restated with plain int64 torch ops: boolean masks and bincounts, on
whatever device the inputs live on.  The reference of tests/test_plstats_*.py; itself held to the reference project's own
intersectionAndUnion by tests/test_plstats_ref.py."""
import torch

ROWS = 13


def table_len(N, bins):
    return ROWS * N + 2 * bins + 1


def _count(cond, key, size):
    """bincount of key over the pixels where cond holds (key is inside [0, size) there)."""
    return torch.bincount(key[cond], minlength=size)[:size].to(torch.int64)


def conf_bin(conf, bins):
    """min((int)(conf * (float)bins), bins - 1) in fp32; a conf that is not >= 0 (negative, NaN) goes to bin 0."""
    conf = conf.to(torch.float32)
    t = conf * torch.tensor(float(bins), dtype=torch.float32, device=conf.device)
    ok = conf >= 0
    top = ok & (t >= float(bins))
    t = torch.where(ok & ~top, t, torch.zeros_like(t))
    return torch.where(top, torch.full_like(t, bins - 1, dtype=torch.int64), t.to(torch.int64))


def pl_stats_ref(mask_w, conf, ign, N, bins, thresh, mc=None, gt=None):
    """The table int64 [13 N + 2 bins + 1] of ONE call on a zeroed table."""
    p, conf, ign = mask_w.reshape(-1), conf.reshape(-1).to(torch.float32), ign.reshape(-1)
    dev, n = p.device, p.numel()
    no = torch.zeros(n, dtype=torch.bool, device=dev)
    thr = torch.tensor(float(thresh), dtype=torch.float32, device=dev)
    v = ign != 255
    k = v & (conf >= thr)
    pv = (p >= 0) & (p < N)
    if mc is not None:
        mc = mc.reshape(-1)
        m = v & (mc >= 0) & (mc < N)
    else:
        mc, m = p, no
    if gt is not None:
        gt = gt.reshape(-1)
        g = v & (gt >= 0) & (gt < N)
    else:
        gt, g = p, no
    rows = [
        _count(v & pv, p, N),                     # 0 pl_area
        _count(k & pv, p, N),                     # 1 plc_area
        _count(m, mc, N),                         # 2 mc_area
        _count(m & (mc == p), mc, N),             # 3 agree
        _count(g, gt, N),                         # 4 gt_area
        _count(g & (gt == p), gt, N),             # 5 pl_inter
        _count(g & pv, p, N),                     # 6 pl_area_gt
        _count(k & g, gt, N),                     # 7 plc_gt_area
        _count(k & g & (gt == p), gt, N),         # 8 plc_inter
        _count(k & g & pv, p, N),                 # 9 plc_area_gt
        _count(m & g, gt, N),                     # 10 mc_gt_area
        _count(m & g & (gt == mc), gt, N),        # 11 mc_inter
        _count(m & g, mc, N),                     # 12 mc_area_gt
    ]
    b = conf_bin(conf, bins)
    rows += [_count(v, b, bins), _count(g & (p == gt), b, bins), torch.tensor([n], dtype=torch.int64, device=dev)]
    return torch.cat(rows)


def triples(table, N):
    """((intersection, prediction area, target area) of the pseudo-labels, of the confident ones, of the guidance)."""
    r = lambda i: table[i * N:(i + 1) * N]
    return (r(5), r(6), r(4)), (r(8), r(9), r(7)), (r(11), r(12), r(10))
