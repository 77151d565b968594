"""svl_confusion_i64 and svl_label_u8_i64 against the int64 restatement tests/evalreport_ref.py: exact equality everywhere --
these are integer counts and byte casts, there is no tolerance.  Sizes around the wave (64) and the block (256), class
counts on both sides of the LDS boundary B = svl_confusion_lds_max_classes(), two trips of the capped grid plus 5, the
contention cases (run-length-coherent and one-class maps) at iou_hist's wrap-test size, labels outside the classes, both
load paths, accumulation, guard bands, bit-equal reruns, the table as a superset of ops.iou_hist, and the refusals."""
import pytest
import torch

import evalreport_ref as R

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = -0x0123456789ABCDEF


def lds_max():
    from semivl_amd import lib as L
    return int(L.load().svl_confusion_lds_max_classes())


def resolve(K):
    return {"B": lds_max(), "B+1": lds_max() + 1}.get(K, K)


def ign(K):
    """The ignore index of the tests: 255, or 2000 where 255 is itself a class (0 <= ignore_index < K is refused)."""
    return 255 if K <= 255 else 2000


def run(pred, target, K, ignore=None, table=None):
    """The kernel on a table between two guard bands -> the guarded buffer."""
    from semivl_amd import ops
    ignore = ign(K) if ignore is None else ignore
    T = R.table_len(K)
    if table is None:
        table = torch.full((GUARD + T + GUARD,), SENTINEL, dtype=torch.int64, device=pred.device)
        table[GUARD:GUARD + T] = 0
    ops.confusion(pred, target, K, ignore, table[GUARD:GUARD + T])
    return table


def check(pred, target, K, ignore=None):
    T = R.table_len(K)
    ignore = ign(K) if ignore is None else ignore
    buf = run(pred, target, K, ignore)
    got, want = buf[GUARD:GUARD + T], R.confusion_ref(pred, target, K, ignore)
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, (bad[:8], got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + T:] == SENTINEL).all(), "guard bands"
    return got


def maps(n, K, seed, dev, run_len=0):
    p, t = R.label_maps(n, K, seed, run_len)
    t[t == 255] = ign(K)
    return p.to(dev), t.to(dev)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 2, 19, 21, 150, "B", "B+1", 256, 1024])
def test_small_sizes_match_the_restatement(dev, n, K):
    K = resolve(K)
    assert 1 <= K <= 1024
    p, t = maps(n, K, 100 * K + n, dev)
    got = check(p, t, K)
    assert int(got.sum()) == int((t != ign(K)).sum())


@pytest.mark.parametrize("run_len", [0, 37])
@pytest.mark.parametrize("K", [21, 150, "B+1"])
def test_two_trips_of_the_capped_grid_plus_five(dev, K, run_len):
    """The grid is capped at 2048 blocks of 256 threads x 2 pixels (fewer blocks for the LDS tables of K = 150: more trips)."""
    K = resolve(K)
    n = 2 * 2048 * 256 * 2 + 5
    p, t = maps(n, K, 5 + K, dev, run_len)
    check(p, t, K)


@pytest.mark.parametrize("K", ["B", "B+1"])
@pytest.mark.parametrize("kind", ["runs", "one_class"])
def test_coherent_maps_at_the_wrap_test_size(dev, K, kind):
    """n = 1.25 * 2^24 + 3 pixels (iou_hist's wrap-test size) of the maps that contend most: runs of one class, and ONE class
    everywhere -- every lane of every wave on one pair key -- on both sides of the LDS boundary."""
    K = resolve(K)
    n = int(2 ** 24 * 1.25) + 3
    if kind == "one_class":
        c = K - 1
        p = torch.full((n,), c, dtype=torch.int64, device=dev)
        got = check(p, p, K)
        assert int(got[c * (K + 1) + c]) == n and int(got.sum()) == n
    else:
        g = torch.Generator(device=dev).manual_seed(17)
        runs = (n + 36) // 37
        t = torch.randint(0, K, (runs,), generator=g, device=dev).repeat_interleave(37)[:n].contiguous()
        p = torch.where(torch.rand(runs, generator=g, device=dev) < 0.8, torch.ones((), dtype=torch.int64, device=dev) * -7,
                        torch.randint(0, K, (runs,), generator=g, device=dev)).repeat_interleave(37)[:n]
        p = torch.where(p == -7, t, p).contiguous()
        t[5::1001] = 255
        got = check(p, t, K)
        assert int(got.sum()) == n - int((t == 255).sum())


def test_labels_outside_the_classes_go_to_the_extra_row_and_column(dev):
    """pred in {-1, K-1, K, 255}; target in {-1, 254, 255, K}: only target == 255 is dropped, the rest lands in row / column K."""
    K = 21
    preds, targets = [-1, K - 1, K, 255, 3], [-1, 254, 255, K, K - 1, 3]
    p = torch.tensor([a for a in preds for _ in targets] * 13, dtype=torch.int64, device=dev)
    t = torch.tensor([b for _ in preds for b in targets] * 13, dtype=torch.int64, device=dev)
    got = check(p, t, K).view(K + 1, K + 1)
    assert int(got.sum()) == 13 * len(preds) * (len(targets) - 1)
    assert int(got[K, K]) == 13 * 3 * 3 and int(got[K - 1, K - 1]) == 13 and int(got[K, K - 1]) == 13 * 3
    assert int(got[K - 1, K]) == 13 * 3 and int(got[3, 3]) == 13 and int(got[:K - 1, :K - 1].sum()) == 13
    # another ignore index: 255 is then an ordinary outside label, -1 is dropped
    got = check(p, t, K, ignore=-1).view(K + 1, K + 1)
    assert int(got.sum()) == 13 * len(preds) * (len(targets) - 1) and int(got[K, K]) == 13 * 3 * 3
    check(p, t, K, ignore=K)
    for Kb in ("B", "B+1", 1024):
        Kb = resolve(Kb)
        p2, t2 = p.clone(), t.clone()
        p2[p == K] = Kb
        p2[p == K - 1] = Kb - 1
        t2[t == K] = Kb
        t2[t == K - 1] = Kb - 1
        check(p2, t2, Kb)


@pytest.mark.parametrize("K", [21, "B+1"])
def test_every_pixel_ignored(dev, K):
    K = resolve(K)
    p, t = maps(777, K, 3, dev)
    t.fill_(ign(K))
    assert not check(p, t, K).any()


@pytest.mark.parametrize("off_p,off_t", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("n", [257, 1030])
@pytest.mark.parametrize("K", [21, "B+1"])
def test_misaligned_maps_take_the_scalar_path(dev, K, n, off_p, off_t):
    """Maps 8 bytes off a 16-byte boundary (both, or only one of them): the scalar loads."""
    K = resolve(K)
    p, t = maps(n + 2, K, 31 + n, dev, run_len=37)
    p, t = p[off_p:off_p + n], t[off_t:off_t + n]
    assert p.is_contiguous() and p.data_ptr() % 16 == 8 * off_p and t.data_ptr() % 16 == 8 * off_t
    check(p, t, K)


@pytest.mark.parametrize("K", [21, 150, "B+1"])
def test_two_calls_accumulate_and_reruns_are_bit_equal(dev, K):
    K = resolve(K)
    T = R.table_len(K)
    (pa, ta), (pb, tb) = maps(9001, K, 41, dev, run_len=37), maps(6007, K, 42, dev)
    want = R.confusion_ref(pa, ta, K, ign(K)) + R.confusion_ref(pb, tb, K, ign(K))
    s = run(pb, tb, K, table=run(pa, ta, K))
    assert torch.equal(s[GUARD:GUARD + T], want)
    assert (s[:GUARD] == SENTINEL).all() and (s[GUARD + T:] == SENTINEL).all()
    assert torch.equal(s, run(pb, tb, K, table=run(pa, ta, K)))


@pytest.mark.parametrize("K", [1, 21, 150, "B+1", 256])
def test_derived_rows_equal_iou_hist(dev, K):
    """The table is a superset of svl_iou_hist_i64's three rows on the same maps (254 / -1 targets, outside predictions)."""
    from semivl_amd import ops
    K = resolve(K)
    p, t = maps(70001, K, 9 + K, dev, run_len=11)
    hist = torch.zeros(3 * K, dtype=torch.int64, device=dev)
    ops.iou_hist(p, t, K, ign(K), hist)
    inter, parea, tarea = R.derived_rows(check(p, t, K), K)
    assert torch.equal(inter, hist[:K]) and torch.equal(parea, hist[K:2 * K]) and torch.equal(tarea, hist[2 * K:])


def test_lds_boundary_setter_does_not_change_results(dev):
    from semivl_amd import lib as L
    lib = L.load()
    B = lds_max()
    p, t = maps(5003, 150, 77, dev, run_len=37)
    want = check(p, t, 150).clone()
    try:
        for b in (0, 149, 150, 201):
            assert lib.svl_set_confusion_lds_max_classes(b) == 0 and lds_max() == b
            assert torch.equal(check(p, t, 150), want)
        assert lib.svl_set_confusion_lds_max_classes(202) == -1 and "160 KB" in L.last_error() and lds_max() == 201
    finally:
        assert lib.svl_set_confusion_lds_max_classes(-1) == 0
    assert lds_max() == B


def test_refusals_leave_the_table_untouched(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    from semivl_amd.ops import _p
    lib = L.load()
    p, t = maps(64, 21, 1, dev)
    table = torch.zeros(R.table_len(21), dtype=torch.int64, device=dev)
    pp, tp, ap = _p(p), _p(t), _p(table)
    bad = [((None, tp, 64, 21, 255, ap), "null"), ((pp, None, 64, 21, 255, ap), "null"), ((pp, tp, 64, 21, 255, None), "null"),
           ((pp, tp, 0, 21, 255, ap), "n = 0 < 1"), ((pp, tp, -5, 21, 255, ap), "n = -5 < 1"),
           ((pp, tp, 64, 0, 255, ap), "K = 0"), ((pp, tp, 64, -2, 255, ap), "K = -2"), ((pp, tp, 64, 1025, 255, ap), "K = 1025"),
           ((pp, tp, 64, 21, 0, ap), "ignore_index = 0"), ((pp, tp, 64, 21, 20, ap), "ignore_index = 20")]
    for args, word in bad:
        assert lib.svl_confusion_i64(*args, None) == -1, word
        err = L.last_error()
        assert "svl_confusion_i64" in err and word in err, err
    torch.cuda.synchronize()
    assert not table.any()
    with pytest.raises(ValueError, match="table"):
        ops.confusion(p, t, 21, 255, table[:-1])
    with pytest.raises(ValueError, match="pred"):
        ops.confusion(p.int(), t, 21, 255, table)
    with pytest.raises(ValueError, match="target"):
        ops.confusion(p, t[:-1], 21, 255, table)
    with pytest.raises(ValueError, match="target"):
        ops.confusion(p, t.cpu(), 21, 255, table)
    with pytest.raises(ValueError, match="pred"):
        ops.confusion(p.view(8, 8).t(), t, 21, 255, table)
    assert not table.any() and ops.confusion_len(21) == 484


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4099])
@pytest.mark.parametrize("off_src,off_dst", [(0, 0), (1, 0), (0, 3), (1, 5)])
def test_label_u8(dev, n, off_src, off_dst):
    """out[i] = (uint8)label[i], numpy's astype(np.uint8): 0, 255, 256 -> 0, -1 -> 255; the 16-byte / 8-byte path, a source
    8 bytes and a destination 3 / 5 bytes off, the n % 8 tail; guard bytes around the output stay."""
    from semivl_amd import ops
    g = torch.Generator().manual_seed(n)
    src = torch.randint(-300, 600, (n + 2,), generator=g)
    src[:4] = torch.tensor([0, 255, 256, -1])[:min(4, n + 2)]
    lab = src.to(dev)[off_src:off_src + n]
    buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[8 + off_dst:8 + off_dst + n]
    assert lab.data_ptr() % 16 == 8 * off_src and out.data_ptr() % 8 == off_dst
    assert ops.label_u8(lab, out=out) is out
    want = torch.from_numpy(src[off_src:off_src + n].numpy().astype("uint8"))
    assert torch.equal(out.cpu(), want)
    assert (buf[:8 + off_dst] == 0xA5).all() and (buf[8 + off_dst + n:] == 0xA5).all(), "guard bytes"
    fresh = ops.label_u8(lab.clone().view(1, n))
    assert fresh.shape == (1, n) and fresh.dtype == torch.uint8 and torch.equal(fresh.view(-1).cpu(), want)


def test_label_u8_refusals(dev):
    from semivl_amd import lib as L
    from semivl_amd import ops
    lab = torch.arange(16, device=dev)
    out = torch.zeros(16, dtype=torch.uint8, device=dev)
    lib = L.load()
    for args, word in (((None, 16, ops._p(out)), "null"), ((ops._p(lab), 16, None), "null"), ((ops._p(lab), 0, ops._p(out)), "n = 0")):
        assert lib.svl_label_u8_i64(*args, None) == -1 and word in L.last_error() and "svl_label_u8_i64" in L.last_error()
    with pytest.raises(ValueError, match="label"):
        ops.label_u8(lab.int())
    with pytest.raises(ValueError, match="out"):
        ops.label_u8(lab, out=out[:-1])
    with pytest.raises(ValueError, match="out"):
        ops.label_u8(lab, out=out.long())
    torch.cuda.synchronize()
    assert not out.any()
