"""Time dcue_crop_tracks over a whole catalogue against the torch route and a plain copy of the same
byte count, and DCUE._item_factors with and without the full-length store; print one JSON line.

  python3 profiles/crop_bench.py [--reps 9] [--out profiles/crop_bench.json]

Shape: BASELINE config 2's catalogue, 200,000 tracks of 1,292 frames x 128 mel bins (30-second
previews), fp16: a 66 GB store, a 6.7 GB [200000][131][128] table.
  crop          dcue_crop_tracks over the whole table, DCUE_CROP_RANDOM (one launch; what DCUE._recrop issues)
  torch         the same windows in torch: index = starts[:, None] + frame_ptr[:-1, None] + arange(131), then
                index_select over the store's frames (the index build is timed: it changes every epoch)
  copy          dst.copy_(src) of a tensor with the table's byte count: the bandwidth yardstick
  factors       DCUE._item_factors(n_iter=10), d = 128, H = 128: with the store bound (ten real passes:
                crop into a scratch table + dcue_item_tower_eval per 8,192 items) and without (one
                pass + dcue_factor_repeat_mean, today's path)
Device events around each call, every route warmed up, the routes alternating in one process; median
and min-max of each. Needs an MI355X: without a GPU it fails.

Agreement (asserted): the kernel's table equals the torch route's bit for bit, at the starts
dcue_crop_starts_host gives.

Not measured here: the kernel alone without its launch (rocprofv3, a run of its own), fp32 stores and
the converting dtype pairs at this scale, ragged catalogues (every track has the same length here),
short tracks, a store larger than HBM, the crop's share of a real training sub-epoch.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))


class _Items:
    """What DCUE._factors_over reads of an item set: the size of the metadata index."""

    def __init__(self, n):
        self.songid2metaindex = range(n)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tracks", type=int, default=200000)
    ap.add_argument("--frames", type=int, default=1292)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--factor-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("crop_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend import _native as nat
    from dcrecommend.nn.dcue import DCUE
    dev = torch.device("cuda:0")
    n, T, W = args.tracks, args.frames, nat.N_FRAMES

    # the store, filled on the device in slices (the values do not matter to a copy; they are fp16 noise)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    data = torch.empty((n * T, nat.N_MELS), dtype=torch.float16, device=dev)
    step = 1 << 20
    for s in range(0, n * T, step):
        e = min(s + step, n * T)
        data[s:e] = torch.randn((e - s, nat.N_MELS), generator=gen, device=dev, dtype=torch.float32).half()
    frame_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * T
    table = torch.empty((n, W, nat.N_MELS), dtype=torch.float16, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = nat.crop_config(nat.CROP_RANDOM, seed=1, draw=3)
    starts = torch.from_numpy(nat.crop_starts_host(cfg, np.full(n, T, dtype=np.int64))).to(dev)
    src = torch.randn((n, W, nat.N_MELS), generator=gen, device=dev, dtype=torch.float32).half()
    dst = torch.empty_like(src)
    arange = torch.arange(W, dtype=torch.int64, device=dev)

    def crop():
        nat.crop_tracks(data, frame_ptr, cfg, table, flags=flags)
        return table

    def torch_route():
        index = ((starts + frame_ptr[:-1])[:, None] + arange).reshape(-1)
        return torch.index_select(data, 0, index).view(n, W, nat.N_MELS)

    def copy():
        dst.copy_(src)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    routes = {"crop": crop, "torch": torch_route, "copy": copy}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():
            times[name].append(timed(fn))
    same = bool(torch.equal(crop(), torch_route()))
    print("agreement: the kernel's table equals the torch route's: %s" % same, file=sys.stderr)
    assert same and not bool(flags.any())
    del src, dst
    torch.cuda.empty_cache()

    # item factors over the whole catalogue, with and without the store
    trainer = DCUE(feature_dim=128, conv_hidden=128, batch_size=64, device="cuda:0", crop="epoch")
    trainer.n_users, trainer.n_items, trainer.epoch_size = 16, n, 64
    trainer._init_nn()
    items = _Items(n)
    trainer._tracks, trainer._tracks_src, trainer._item_meta = table, items, np.arange(n, dtype=np.int64)

    def factors(store):
        trainer._store = (data, frame_ptr) if store else None
        trainer._item_factors(items, n_iter=10)

    for name, store in (("factors_store", True), ("factors_table", False)):
        factors(store)
        torch.cuda.synchronize()
        times[name] = []
    for _ in range(args.factor_reps):
        for name, store in (("factors_store", True), ("factors_table", False)):
            times[name].append(timed(lambda: factors(store)))
    assert bool(torch.isfinite(trainer.item_factors).all())

    def stat(name):
        v = times[name]
        return {"median": float(np.median(v)), "min": min(v), "max": max(v)}

    med = {name: float(np.median(v)) for name, v in times.items()}
    out_bytes = n * W * nat.N_MELS * 2
    res = {
        "bench": "crop", "device": torch.cuda.get_device_name(0),
        "shape": {"tracks": n, "frames": T, "dtype": "fp16", "store_bytes": n * T * nat.N_MELS * 2,
                  "table_bytes": out_bytes, "model": {"feature_dim": 128, "conv_hidden": 128}, "n_iter": 10},
        "reps": args.reps, "factor_reps": args.factor_reps, "warmup": args.warmup,
        "ms": {name: stat(name) for name in times},
        # a copy reads and writes the byte count once each, and so does the crop
        "crop_gbps_read_plus_write": 2 * out_bytes / (med["crop"] * 1e-3) / 1e9,
        "copy_gbps_read_plus_write": 2 * out_bytes / (med["copy"] * 1e-3) / 1e9,
        "copy_over_crop": med["copy"] / med["crop"],
        "torch_over_crop": med["torch"] / med["crop"],
        "factors_store_over_table": med["factors_store"] / med["factors_table"],
        "crop_share_of_factors_store": 10 * med["crop"] / med["factors_store"],
        "agreement_bitwise": same,
        "not_measured": ["the kernel alone without its launch (rocprofv3)", "fp32 stores and the converting dtype pairs",
                         "ragged catalogues and short tracks at this scale", "a store larger than HBM",
                         "the crop's share of a real training sub-epoch"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
