"""The shapes tests/test_gpu_shapes.py runs against the fp64 oracle, and the variant keys of a shape's
launches (dcue_debug_launch_shape). tests/test_launch_shapes_cpu.py asserts that these cases reach
every key a shape can select, so a planner threshold that moves must bring a case along. No GPU is
touched at import."""

CATALOGUE, GATHER = 0, 1  # dcue_batch.layout
BN = "truedcuemel1dbn"

# (layout, model_type, B, N, d, H). Catalogue: M = B (1 + N); in-batch (gather): M = B.
CASES = [("catalogue", BN, B, N, 32, 32) for B, N in
         ((1, 1), (1, 2), (1, 4), (1, 16), (3, 10), (1, 62), (5, 12), (1, 126), (43, 2), (31, 7), (83, 2),
          (71, 6), (27, 18), (93, 10), (64, 15), (683, 2), (128, 31), (100, 40), (128, 63))]
CASES += [("catalogue", BN, 3, 42, 128, 128), ("catalogue", BN, 1, 256, 128, 128)]
CASES += [("inbatch", BN, B, N, 32, 32) for B, N in ((2, 1), (3, 40), (33, 16), (65, 31), (129, 32), (257, 15))]
# d = 256: the fc rides in the one-item-per-workgroup item gradient (k_item_grad)
CASES += [("catalogue", BN, 3, 2, 256, 32)]
# the other wired towers at a ragged M
CASES += [("catalogue", mt, 5, 12, 32, 32) for mt in ("truedcuemel1d", "truedcuemel1dres", "truedcuemel1dresbn")]

# Added until test_launch_shapes_cpu.py's closure passed: mostly the full-last-tile / one-chunk
# twins of the ragged variants above, the thresholds of layers 3-5 at large M, and the variants only
# the d = 256 width (two column blocks on conv 5) or a res tower (no fc in the item gradient) selects.
CASES += [("catalogue", BN, B, N, 32, 32) for B, N in
          ((2, 1), (16, 1), (32, 1), (64, 1), (144, 1), (513, 1), (688, 5), (878, 6))]
CASES += [("catalogue", BN, B, N, 128, 128) for B, N in ((1, 1), (1, 2), (6, 1))]
CASES += [("catalogue", BN, 688, 2, 256, 32), ("catalogue", BN, 717, 4, 256, 32)]
CASES += [("catalogue", "truedcuemel1dres", B, N, 32, 32) for B, N in ((128, 1), (1, 256), (264, 1), (205, 4))]

# the (H, d) the invariants are checked at, and M's range
WIDTHS = ((32, 32), (128, 128), (256, 128))
M_MAX = 8192
# in-batch steps have M = B items; the fused score kernel takes at most 1,024 rows and 1,024 negatives
B_MAX = N_MAX = 1024


def catalogue_batch(M):
    """(B, N) of a catalogue training step with M = B (1 + N) items, N >= 1 (a step without
    negatives has no loss) and B, N within the score kernel's limits; None where M has none."""
    for copies in range(2, min(M, N_MAX + 1) + 1):
        if M % copies == 0 and M // copies <= B_MAX:
            return M // copies, copies - 1
    return None


def step_batches(M):
    """The (layout, B, N) of the training steps that run the item tower on M items."""
    bn = catalogue_batch(M)
    if bn:
        yield (CATALOGUE,) + bn
    if 2 <= M <= B_MAX:
        yield GATHER, M, 1


def case_id(c):
    layout, mt, B, N, d, H = c
    return "%s-%s-B%d-N%d-d%d-H%d" % (layout, mt[len("truedcuemel1d"):] or "plain", B, N, d, H)


def case_items(c):
    layout, _, B, N, _, _ = c
    return B if layout == "inbatch" else B * (1 + N)


def shape_of(nat, c):
    layout, mt, B, N, d, H = c
    dims = nat.make_dims(H, d, 300, 50, mt)
    return nat.launch_shape(dims, GATHER if layout == "inbatch" else CATALOGUE, B, N, case_items(c))


def conv_keys(shape):
    """Variant keys of a shape's M-dependent launches: per layer (kernel, TW, DEEP, f16, last tile
    ragged, a tile spans two items) for the row-GEMM convs, (kernel, several chunks, short last chunk)
    for the weight gradients, and the item gradient's (kernel, IT, WLDS, short last workgroup)."""
    keys = set()
    for kind in ("fwd", "dgrad"):
        for l, (tw, deep, f16, last, spans) in shape[kind].items():
            keys.add((kind, l, tw, deep, f16, last != 0, spans))
    for l, (kernel, nchunk, rpc, last) in shape["wgrad"].items():
        if kernel is not None:
            keys.add(("wgrad", l, kernel, nchunk > 1, last < rpc))
    _, kernel, it, wlds, last = shape["tail"]
    keys.add(("item_grad", kernel, it, wlds, last < it))
    return keys


def score_key(shape):
    return ("score", shape["tail"][0])


def keys_of(shape):
    return conv_keys(shape) | {score_key(shape)}
