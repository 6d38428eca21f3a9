"""The device half of the strip schedule restated in numpy: cost classes from records, the classes
of a frame with a skip mask, the motion floor, and the eight lists from class bytes and the nine cumulative shares.  Integer
arithmetic throughout, so the GPU tests compare exactly.  Written from the design's wording, one strip or one class at a time:
nothing here knows about waves, chunks or ballots."""
import numpy as np

COST_SHIFT = 2                   # a class is 4 steps wide (svo_device.h: kCostShift)
COST_CLASSES = 128 >> COST_SHIFT  # kCostClasses
N_LISTS = 8
OUT = 0xFF                       # the class byte of a strip that is in no list
LONG_CLASS = 64 >> COST_SHIFT    # a strip with a ray of 64 steps or more: what the motion floor counts
LEARN_FRAMES = 16                # kBalanceLearnFrames


def list_cap(n_strips):
    """entries reserved per list (svo_device.h: order_list_cap)"""
    return (n_strips + 3) // 4 + COST_CLASSES


def steps_of(records):
    return (np.asarray(records)["info"] & 0xFF).astype(np.int64)


def cost_classes(records, bw_log2=None, shadow=None):
    """Class byte per 64-item strip: min(max steps >> COST_SHIFT, COST_CLASSES - 1), the steps of an item being its record's
    plus, with `shadow`, its shadow record's.  bw_log2 None: explicit rays, `records` flat, strip s = items 64 s .. 64 s + 63 (a
    ragged last strip holds fewer).  Else pixel frames: `records` is (h, w) or (n_rects, h, w), every rectangle cut into blocks
    2^bw_log2 wide and 64 >> bw_log2 high, row-major, rectangle after rectangle; blocks on the right and bottom edges may be
    partial -- the pixels they do not have count nothing."""
    steps = steps_of(records)
    if shadow is not None:
        steps = steps + steps_of(shadow).reshape(steps.shape)
    if bw_log2 is None:
        steps = steps.reshape(-1)
        n = (steps.size + 63) // 64
        padded = np.zeros(n * 64, dtype=np.int64)
        padded[:steps.size] = steps
        most = padded.reshape(n, 64).max(axis=1) if n else padded
    else:
        if steps.ndim == 2:
            steps = steps[None]
        bw, bh = 1 << bw_log2, 64 >> bw_log2
        rects, h, w = steps.shape
        bpr, bpc = -(-w // bw), -(-h // bh)
        padded = np.zeros((rects, bpc * bh, bpr * bw), dtype=np.int64)
        padded[:, :h, :w] = steps
        most = padded.reshape(rects, bpc, bh, bpr, bw).max(axis=(2, 4)).reshape(-1)
    return np.minimum(most >> COST_SHIFT, COST_CLASSES - 1).astype(np.uint8)


def skip_classes(skip, n_items, prev=None):
    """Classes of a frame of explicit rays with a skip mask (non-zero byte: no ray in the slot): OUT for a strip whose every
    slot below n_items is skipped, else the class the strip had before (`prev`), or 0 without one."""
    skip = np.asarray(skip).reshape(-1)[:n_items]
    n = (n_items + 63) // 64
    out = np.zeros(n, dtype=np.uint8)
    for s in range(n):
        slots = skip[64 * s:min(64 * s + 64, n_items)]
        out[s] = OUT if (slots != 0).all() else (prev[s] if prev is not None else 0)
    return out


def motion_option(option):
    """SVO_OPT_SCHEDULE_MOTION -> (radius, min_count, floor_class): class floor in units of 8 steps | radius << 8 | count << 12"""
    return (option >> 8) & 15, (option >> 12) & 255, ((option & 15) << 3) >> COST_SHIFT


def danger_floor(classes, bpr, radius, min_count, floor_class):
    """The motion floor: a strip below floor_class with at least min_count long strips (class >= LONG_CLASS) among the
    (2 radius + 1)^2 blocks around it that lie on the screen, itself included, is given floor_class."""
    classes = np.asarray(classes)
    n = classes.size
    rows = -(-n // bpr)
    grid = np.zeros((rows, bpr), dtype=bool)
    grid.reshape(-1)[:n] = classes >= LONG_CLASS
    out = classes.copy()
    for s in range(n):
        if classes[s] >= floor_class:
            continue
        y, x = divmod(s, bpr)
        near = grid[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1].sum()
        if near >= min_count:
            out[s] = floor_class
    return out


def rank_order(n_strips, bpr):
    """the strips in the order a class ranks them: column by column of the block grid when bpr != 0, else as numbered"""
    if bpr == 0:
        return np.arange(n_strips)
    assert n_strips % bpr == 0
    return np.arange(n_strips).reshape(n_strips // bpr, bpr).T.reshape(-1)


def build_lists(classes, n_strips, bpr, shares, cap):
    """(lengths, lists): list k gets, class by class from the most expensive down, the strips of the class whose rank r inside it
    satisfies bound[k] <= r < bound[k + 1], bound[k] = (total * shares[k] + 32768) >> 16 (shares: nine cumulative 16-bit
    fractions, 0 .. 65536).  Strips of class OUT are in no list.  Raises when a list would not fit `cap` entries."""
    classes = np.asarray(classes)[:n_strips]
    shares = [int(v) for v in shares[:N_LISTS + 1]]
    assert shares[0] == 0 and shares[N_LISTS] == 65536
    order = rank_order(n_strips, bpr)
    lists = [[] for _ in range(N_LISTS)]
    for c in range(COST_CLASSES - 1, -1, -1):
        members = order[classes[order] == c]
        total = members.size
        bound = [(total * s + 32768) >> 16 for s in shares]
        for k in range(N_LISTS):
            lists[k].extend(members[bound[k]:bound[k + 1]].tolist())
    for k, l in enumerate(lists):
        if len(l) > cap:
            raise OverflowError(f"list {k} holds {len(l)} strips, {cap} reserved ({n_strips} strips, shares {shares})")
    return np.array([len(l) for l in lists], dtype=np.uint32), lists


def check_shares(bal):
    """what every state of the balance words must satisfy (svo_sched.h: balance_share_step)"""
    s = [int(v) for v in bal[:N_LISTS + 1]]
    assert s[0] == 0 and s[N_LISTS] == 65536, s
    parts = [b - a for a, b in zip(s, s[1:])]
    assert min(parts) > 0, f"shares not strictly increasing: {s}"
    assert max(parts) <= 16384, f"a list's share exceeds 2/8: {parts}"
    return parts


def check_stored_lists(status, what="", motion=0x1204):
    """check_lists for the complete lists a post pass built: from the measured classes, or -- when the camera had moved since the
    frame before, whoever traced that one -- from their floored copy, which is held to danger_floor first.  motion: the
    context's SVO_OPT_SCHEDULE_MOTION.  Returns the classes the lists were built from."""
    assert not status["order_filtered"], f"{what}: the lists are a filtered frame's"
    used = status["classes"]
    if status["floored"]:
        used = danger_floor(status["classes"], status["bpr"], *motion_option(motion))
        assert np.array_equal(status["classes_now"], used), f"{what}: floored classes differ"
    check_lists(status, used, what)
    return used


def check_lists(status, classes, what=""):
    """The device's lists (Gpu.schedule_status) against build_lists over `classes` and the shares in the status' balance words;
    and, without the restatement: every strip with a class other than OUT is in exactly one list, classes never increase along a
    list, no list is longer than the cap."""
    n, cap, bpr = status["n_strips"], status["cap"], status["bpr"]
    classes = np.asarray(classes)
    assert classes.size == n, f"{what}: {classes.size} classes for {n} strips"
    lengths = status["lengths"].astype(np.int64)
    assert lengths.max() <= cap, f"{what}: lengths {lengths.tolist()} beyond the cap {cap}"
    got = [status["lists"][k, :lengths[k]].astype(np.int64) for k in range(N_LISTS)]
    listed = np.concatenate(got)
    assert listed.size == 0 or listed.max() < n, f"{what}: a list names strip {listed.max()} of {n}"
    seen = np.bincount(listed, minlength=n)
    want_seen = (classes != OUT).astype(np.int64)
    bad = np.flatnonzero(seen != want_seen)
    assert bad.size == 0, f"{what}: {bad.size} strips not listed exactly once (or listed though left out); first {bad[:8].tolist()}: listed {seen[bad[:8]].tolist()} times"
    for k, l in enumerate(got):
        assert (np.diff(classes[l].astype(np.int64)) <= 0).all(), f"{what}: classes increase along list {k}"
    want_len, want = build_lists(classes, n, bpr, status["balance"], cap)
    assert lengths.tolist() == want_len.tolist(), f"{what}: lengths {lengths.tolist()}, want {want_len.tolist()}"
    for k in range(N_LISTS):
        assert got[k].tolist() == want[k], f"{what}: list {k} differs from the restatement"
