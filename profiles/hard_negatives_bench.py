"""Time what hard negatives add to a batch's preparation (the P-wide draw and dcue_select_negatives)
beside a torch route of the same selection, at BASELINE config 2's sampler shape, and one catalogue
sub-epoch of the trainer with and without them; print one JSON line.

  python3 profiles/hard_negatives_bench.py [--step-ms MS] [--out profiles/hard_negatives_bench.json]

Sampler shape: a 200,000-song split, 100,000 users with about 50 plays each over Zipf-like song
popularity, 64 samples per call, N = 20, H = 10, randn factors of d = 100, P in {40, 160, 640}:
  draw      dcue_sample_catalogue, P draws per row on the global stream (what _Negatives.draw issues)
  draw_n    the same with N draws per row: today's cost, for scale
  select    dcue_select_negatives over the pool
  torch     gather + bmm + topk: item_feat[pool] ([B, P, d]), the cosines by bmm and two norms, topk(H).
            It stops there -- no first-occurrence rule, no fill, no flags -- so it is a floor for a torch
            route, not an equivalent.
Each figure is the device-event time of `--inner` back-to-back calls over different user batches divided
by their number, the routes alternating in one process after a warm-up; median and min-max over `--reps`.
Needs an MI355X: without a GPU it fails.

The condition this measurement is for: the trainer prepares a batch on its sampling stream while the
two steps before it run, so draw + select stays off the critical path as long as it takes less than one
catalogue training step. --step-ms is that step's time for the parent commit (bench.py --full --modes
catalogue --gpu-only, the catalogue object's ms_per_step), measured by the caller on the same machine
in the same session; it is recorded beside the times, with the verdict per P.

Sub-epoch: DCUE._train_epoch over a synthetic catalogue (--epoch-songs songs, --epoch-users users,
--epoch-pairs plays, random fp16 tracks bound without files), B = 64, N = 20, H = 10, d = 100, conv_hidden = 128; wall time
to the end of the device work, neg_pool=None and neg_pool=160 alternating after a warm-up of each.

Agreement (asserted): the first batch's selection passes tests/hard_negatives_reference.py's tolerance
check against fp64 scores at every P.

Not measured here: any effect on validation mAP or on the loss curve; the share of sampled negatives
with an active hinge term, before or after, on a real catalogue (none exists here: the factors are
random, the tracks noise); the kernels alone without their launches (rocprofv3, a run of its own);
weighted ('popularity') pools; other B, N, H and d; P = 1024; users with thousands of plays.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOT_MEASURED = ["any effect on validation mAP or the loss curve",
                "the hinge-active share of the negatives on a real catalogue (random factors, noise tracks here)",
                "the kernels alone without their launches (rocprofv3)", "weighted ('popularity') pools",
                "other B, N, H and d", "P = 1024", "users with thousands of plays"]


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def sampler_part(args, torch, nat, dev):
    import hard_negatives_reference as R
    from dcrecommend.datasets.csr import user_split_ranks
    n, n_users, B, N, H, d = args.songs, args.users, args.batch, args.neg, args.hard, args.dim
    rs = np.random.RandomState(args.seed)
    p = 1.0 / np.arange(1, n + 1) ** 0.8  # Zipf-like song popularity
    rs.shuffle(p)
    n_pairs = n_users * args.plays
    uidx = rs.randint(0, n_users, n_pairs)
    sidx = rs.choice(n, n_pairs, p=p / p.sum())
    split = np.arange(n, dtype=np.int64)
    indptr, ranks = user_split_ranks(uidx, sidx, n_users, split)
    uf, itf = rs.randn(n_users, d).astype(np.float32), rs.randn(n, d).astype(np.float32)

    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    split_d, indptr_d, ranks_d, uf_d, itf_d = to(split), to(indptr), to(ranks), to(uf), to(itf)
    n_batches = args.inner * (args.reps + args.warmup)
    users_h = rs.randint(0, n_users, (n_batches, B)).astype(np.int64)
    users_d = to(users_h)
    mt = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=dev)
    lib, stream = nat.lib(), nat.stream_handle(dev)
    nat.check(lib.dcue_mt_seed(nat.ptr(mt), 77, stream), "dcue_mt_seed")
    out = torch.empty((B, N), dtype=torch.int64, device=dev)
    hard = torch.empty(B, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)

    def draw(k, buf):
        nat.check(lib.dcue_sample_catalogue(nat.ptr(mt), 0, 0, nat.ptr(split_d), n, nat.ptr(indptr_d), nat.ptr(ranks_d),
                                            nat.ptr(users_d[k]), B, buf.shape[1], nat.ptr(buf), stream),
                  "dcue_sample_catalogue")

    def torch_route(k, pool):
        c = itf_d[pool]                                    # [B, P, d]
        u = uf_d[users_d[k]]                               # [B, d]
        s = torch.bmm(c, u.unsqueeze(2)).squeeze(2)
        s = s / (u.norm(dim=1, keepdim=True).clamp_min(1e-8) * c.norm(dim=2).clamp_min(1e-8))
        return torch.topk(s, H, dim=1)

    per_p, agree = {}, True
    for P in args.pools:
        pool = torch.empty((B, P), dtype=torch.int64, device=dev)
        draw(0, pool)
        nat.select_negatives(uf_d, itf_d, users_d[0], pool, N, H, out, hard, flags)
        try:
            R.check_against(uf, itf, users_h[0], pool.cpu().numpy(), N, H, out.cpu().numpy(), hard.cpu().numpy())
        except AssertionError as e:
            agree = False
            print("agreement FAILED at P = %d: %s" % (P, e), file=sys.stderr)
        routes = {"draw": lambda k: draw(k, pool), "draw_n": lambda k: draw(k, out),
                  "select": lambda k: nat.select_negatives(uf_d, itf_d, users_d[k], pool, N, H, out, hard, flags),
                  "torch": lambda k: torch_route(k, pool)}
        times = {name: [] for name in routes}
        for rep in range(args.warmup + args.reps):
            for name, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(args.inner):
                    fn(rep * args.inner + i)
                b.record()
                b.synchronize()
                if rep >= args.warmup:
                    times[name].append(a.elapsed_time(b) / args.inner)
        ms = {name: stats(v) for name, v in times.items()}
        both = ms["draw"]["median"] + ms["select"]["median"]
        worst = ms["draw"]["max"] + ms["select"]["max"]
        per_p[str(P)] = {"ms_per_call": ms, "draw_plus_select_ms": both, "draw_plus_select_worst_ms": worst,
                         "draw_share": ms["draw"]["median"] / both,
                         "select_over_torch": ms["select"]["median"] / ms["torch"]["median"],
                         "below_one_parent_step": None if args.step_ms is None else bool(worst < args.step_ms)}
    assert agree
    shape = {"split_songs": n, "users": n_users, "mean_split_plays_per_user": float(len(ranks)) / n_users,
             "samples": B, "neg": N, "hard": H, "d": d, "pools": list(args.pools)}
    return shape, per_p, agree


class _Catalogue:
    """What DCUE's factor passes read of an item dataset: every song has a metadata row and a track."""

    def __init__(self, ds):
        self.user_index = ds.user_index
        self.songid2metaindex = {s: i for s, i in ds.item_index.items()}


def epoch_part(args, torch, dev):
    import pandas as pd
    from dcrecommend import _native as nat
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.nn.dcue import DCUE
    rs = np.random.RandomState(args.seed + 1)
    n, n_users, B, N = args.epoch_songs, args.epoch_users, args.batch, args.neg
    pairs = np.unique(np.stack([rs.randint(0, n_users, args.epoch_pairs), rs.randint(0, n, args.epoch_pairs)], 1), axis=0)
    trip = pd.DataFrame({"user_id": ["u%06d" % u for u in pairs[:, 0]], "song_id": ["s%06d" % s for s in pairs[:, 1]],
                         "score": np.ones(len(pairs), dtype=np.float32)})
    songs = sorted(set(trip["song_id"]))
    meta = pd.DataFrame({"idx": np.arange(len(songs)), "song_id": songs, "data_mel": [""] * len(songs)})
    state = np.random.get_state()
    ds = DCUEDataset(trip.copy(), meta, neg_samples=N, split="train")
    items = _Catalogue(ds)
    gen = torch.Generator(device=dev).manual_seed(5)
    tracks = torch.randn((len(ds.item_index), nat.N_FRAMES, nat.N_MELS), generator=gen, device=dev).half()

    def trainer(neg_pool):
        tr = DCUE(feature_dim=args.dim, conv_hidden=args.hidden, batch_size=B, neg_batch_size=N, lr=1e-5, device=dev,
                  neg_pool=neg_pool, neg_hard=None if neg_pool is None else args.hard)
        tr.n_users, tr.n_items = len(ds.user_index), len(ds.item_index)
        tr.epoch_size = int(int(np.ceil(len(ds) / 10)) // B) * B
        tr.train_data, tr.item_data = ds, items
        torch.manual_seed(3)
        tr._init_nn()
        tr._tracks, tr._tracks_src, tr._store = tracks, items, None
        tr._item_meta = np.arange(len(ds.item_index), dtype=np.int64)
        tr._user_factors(items)
        tr._item_factors(items)
        return tr

    modes = {"none": trainer(None), "pool_%d" % args.epoch_pool: trainer(args.epoch_pool)}
    times, steps = {k: [] for k in modes}, None
    for rep in range(1 + args.epoch_reps):
        for name, tr in modes.items():
            np.random.seed(100 + rep)
            torch.manual_seed(100 + rep)
            loader = tr._batch_loaders(ds, k=10)[0]
            tr.scheduler.step()  # as fit does before every sub-epoch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_rows, loss = tr._train_epoch(loader)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            steps = n_rows // B
            assert np.isfinite(loss)
            if rep >= 1:
                times[name].append(dt * 1e3)
    np.random.set_state(state)
    res = {name: dict(stats(v), ms_per_step=float(np.median(v)) / steps) for name, v in times.items()}
    a, b = res["none"]["median"], res["pool_%d" % args.epoch_pool]["median"]
    return {"shape": {"songs": len(ds.item_index), "users": len(ds.user_index), "train_rows": len(ds),
                      "split_songs": int(len(ds.split_items())), "batch": B, "neg": N, "hard": args.hard,
                      "pool": args.epoch_pool, "d": args.dim, "conv_hidden": args.hidden, "steps": steps,
                      "tracks": "random fp16, bound without files"},
            "reps": args.epoch_reps, "wall_ms": res, "pool_over_none": b / a}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--songs", type=int, default=200000)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--plays", type=int, default=50, help="mean plays per user")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--neg", type=int, default=20)
    ap.add_argument("--hard", type=int, default=10)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--pools", type=int, nargs="+", default=[40, 160, 640])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--epoch-songs", type=int, default=20000)
    ap.add_argument("--epoch-users", type=int, default=5000)
    ap.add_argument("--epoch-pairs", type=int, default=300000)
    ap.add_argument("--epoch-pool", type=int, default=160)
    ap.add_argument("--epoch-reps", type=int, default=3)
    ap.add_argument("--no-epoch", action="store_true", help="skip the sub-epoch part")
    ap.add_argument("--step-ms", type=float, help="one catalogue training step of the parent commit, same session")
    ap.add_argument("--step-source", default="bench.py --full --modes catalogue --gpu-only, catalogue ms_per_step")
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hard_negatives_bench: no GPU found (this measurement runs only on the MI355X)")
    from dcrecommend import _native as nat
    dev = torch.device("cuda:0")
    shape, per_p, agree = sampler_part(args, torch, nat, dev)
    step = args.step_ms
    failing = [int(P) for P, r in per_p.items() if r["below_one_parent_step"] is False]
    res = {"bench": "hard_negatives", "device": torch.cuda.get_device_name(0), "shape": shape,
           "reps": args.reps, "inner": args.inner, "warmup": args.warmup, "by_pool": per_p,
           "parent_catalogue_step_ms": step, "parent_catalogue_step_source": args.step_source if step is not None else None,
           # the condition: the slowest draw + the slowest select seen stay below one parent step
           "condition_holds_for_every_pool": None if step is None else not failing,
           "condition_fails_from_pool": min(failing) if failing else None,
           "agreement_within_tau": agree,
           "sub_epoch": None if args.no_epoch else epoch_part(args, torch, dev),
           "not_measured": NOT_MEASURED}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
