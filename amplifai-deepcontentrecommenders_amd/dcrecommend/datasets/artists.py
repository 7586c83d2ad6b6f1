"""Who recorded a song, for artist-aware serving: the item -> group map nn.rank.GroupCap and
TopK(max_per_group=) read, and the exclusion rows of "not by the same artist" / "artists this user has
not heard" in dcue_topk's CSR format (each row sorted, no repeats).

The reference names artists only as DCUEDataset(song_artist_map=...), a {song_id: artist} dict that
drives its artist split; the same dict is what these helpers take.
"""
import numpy as np
from scipy.sparse import csr_matrix, diags


def artist_groups(item_index, song_artist_map):
    """(group_of int32 [n_items], artist_names): group_of[item_index[song]] is the rank of the song's
    artist among the artists PRESENT -- those of at least one song of item_index -- in sorted order, and
    artist_names[g] is the artist of group g. A song without an entry in the map (or mapped to None) is
    ungrouped: -1. item_index: {song_id: item index}, the indices 0 .. n_items - 1."""
    n = len(item_index)
    if sorted(item_index.values()) != list(range(n)):
        raise ValueError("item_index must map the songs onto 0..%d, each index once" % (n - 1))
    artist_of = [None] * n
    for song, i in item_index.items():
        artist_of[i] = song_artist_map.get(song)
    names = sorted({a for a in artist_of if a is not None})
    rank_of = {a: g for g, a in enumerate(names)}
    group_of = np.array([-1 if a is None else rank_of[a] for a in artist_of], dtype=np.int32).reshape(n)
    return group_of, names


def _membership(group_of, n_groups):
    """Sparse [n_items, n_groups] indicator of item -> group; ungrouped items have empty rows."""
    group_of = np.asarray(group_of, dtype=np.int64).reshape(-1)
    has = np.flatnonzero(group_of >= 0)
    return csr_matrix((np.ones(len(has), np.int64), (has, group_of[has])), shape=(len(group_of), n_groups))


def _as_csr(ptr_idx, n_cols):
    ptr, idx = ptr_idx
    ptr = np.asarray(ptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)[:ptr[-1]]
    return csr_matrix((np.ones(len(idx), np.int64), idx, ptr), shape=(len(ptr) - 1, n_cols))


def artist_exclusion_csr(group_of, played=None, seen=None):
    """(int64 pointers, int32 indices) of per-row exclusion lists over item indices, each row sorted and
    without repeats (dcue_topk's exclusion CSR), from sparse products of the item -> artist indicator:

      played is None          one row per song: the OTHER songs of its artist (an ungrouped song: none).
      played = (ptr, idx)     one row per user, over the user's played songs (a CSR over item indices):
                              every song by any artist of a played song.

    seen = (ptr, idx), a CSR with the same rows, is united with the result: the songs themselves
    (nn.rank.identity_csr) for item-to-item lists, the users' played songs for recommendations."""
    group_of = np.asarray(group_of, dtype=np.int64).reshape(-1)
    n = len(group_of)
    if n and group_of.min() < -1:
        raise ValueError("group_of holds a group id below -1")
    A = _membership(group_of, int(group_of.max()) + 1 if n else 0)
    if played is None:
        M = (A @ A.T - diags((group_of >= 0).astype(np.int64))).tocsr()  # a song has one artist: diagonal 1
        M.eliminate_zeros()
    else:
        M = ((_as_csr(played, n) @ A) @ A.T).tocsr()
    if seen is not None:
        S = _as_csr(seen, n)
        if S.shape != M.shape:
            raise ValueError("seen has %d rows, the exclusion %d" % (S.shape[0], M.shape[0]))
        M = (M + S).tocsr()
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32)
