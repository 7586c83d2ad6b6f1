"""Host formulas of popularity-aware serving: from per-item play counts, the scaled
log-popularity a serving prior is built from, the self-information novelty averages, and the long-tail
bytes. All of it float64 numpy on the host; the device only adds, counts and divides what is made here."""
import numpy as np

HEAD_MASS = 0.8


def item_counts(item_index, counts):
    """int64 [n_items] over item indices from a {song_id: count} dict; songs without an entry count 0.
    A negative or non-integer count raises ValueError."""
    out = np.zeros(len(item_index), dtype=np.int64)
    for song, i in item_index.items():
        c = counts.get(song, 0)
        if int(c) != c or c < 0:
            raise ValueError("the count of song %r must be a non-negative integer, got %r" % (song, c))
        out[int(i)] = int(c)
    return out


def log_popularity(counts):
    """z_i = log2(1 + n_i) / log2(1 + max n) in [0, 1] (zeros where no item has a count)."""
    n = np.asarray(counts, dtype=np.float64)
    top = float(n.max()) if len(n) else 0.0
    return np.log2(1.0 + n) / np.log2(1.0 + top) if top > 0 else np.zeros(len(n), dtype=np.float64)


def self_information(counts):
    """v_i = -log2((n_i + 1) / sum_j (n_j + 1)): the bits of surprise of meeting item i among all plays,
    add-one smoothed so that an unplayed item has a finite value."""
    n = np.asarray(counts, dtype=np.float64) + 1.0
    return -np.log2(n / n.sum())


def tail_bytes(counts, head_mass=HEAD_MASS):
    """uint8 [n]: 0 for the head, 1 for the long tail. With the items sorted by count descending (ties by
    index ascending), the head is the shortest prefix holding at least head_mass of all counts."""
    n = np.asarray(counts, dtype=np.int64)
    if not 0.0 <= float(head_mass) <= 1.0:
        raise ValueError("head_mass must be in [0, 1], got %r" % (head_mass,))
    order = np.lexsort((np.arange(len(n)), -n))
    cum = np.cumsum(n[order])
    total = int(cum[-1]) if len(n) else 0
    head = int(np.searchsorted(cum.astype(np.float64), float(head_mass) * total, side="left")) + 1 if total > 0 else 0
    if float(head_mass) * total <= 0:
        head = 0
    tail = np.ones(len(n), dtype=np.uint8)
    tail[order[:head]] = 0
    return tail


def popularity_prior(z, beta):
    """float32(beta * z_i): one rounding of the float64 product."""
    return (float(beta) * np.asarray(z, dtype=np.float64)).astype(np.float32)
