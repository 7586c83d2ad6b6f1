"""Time one batch's popularity-weighted negative draw (dcue_sample_catalogue_weighted) beside the
uniform draw (dcue_sample_catalogue) at BASELINE config 2's sampler shape; print one JSON line.

  python3 profiles/weighted_sampler_bench.py [--step-ms MS] [--out profiles/weighted_sampler_bench.json]

Shape: a 200,000-song split, 100,000 users with about 50 plays each over Zipf-like song popularity,
64 samples x N = 20 per call, weights popularity_weights(count, 0.75).
  weighted_stream   one call on the global stream (one workgroup: what _Negatives.draw issues per batch)
  uniform_stream    dcue_sample_catalogue on the same users, the same way
  weighted_reseed   one call of the reseed form (one workgroup per sample)
Each figure is the device-event time of `--inner` back-to-back calls over different user batches divided
by their number, the routes alternating in one process after a warm-up; median and min-max over `--reps`.
Needs an MI355X: without a GPU it fails.

The condition this measurement is for: the trainer draws a batch's negatives two steps ahead on its
sampling stream, so the draw stays off the critical path as long as one call takes less than one
catalogue training step. --step-ms is that step's time (bench.py's catalogue ms_per_step), measured by
the caller on the same machine in the same session; it is recorded beside the three times.

Agreement (asserted): the first batch equals the numpy definition (tests/weighted_sampler_reference.py).

Not measured here: the kernels alone without their launches (rocprofv3, a run of its own), other N and
batch sizes, users with thousands of plays (lists past the LDS stage), total weights near 2^32 (more
rejections per draw), the draw's effect on a real sub-epoch's wall time, anything about ranking quality.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--songs", type=int, default=200000)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--plays", type=int, default=50, help="mean plays per user")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--neg", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-ms", type=float, help="one catalogue training step of the parent commit, same session")
    ap.add_argument("--step-source", default="bench.py --modes catalogue, ms_per_step")
    ap.add_argument("--out")
    args = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("weighted_sampler_bench: no GPU found (this measurement runs only on the MI355X)")
    import weighted_sampler_reference as R
    from dcrecommend import _native as nat
    from dcrecommend.datasets.csr import popularity_weights, user_split_ranks, weighted_split_tables
    dev = torch.device("cuda:0")
    n, n_users, B, N = args.songs, args.users, args.batch, args.neg

    rs = np.random.RandomState(args.seed)
    p = 1.0 / np.arange(1, n + 1) ** 0.8  # Zipf-like song popularity
    rs.shuffle(p)
    n_pairs = n_users * args.plays
    uidx = np.concatenate([rs.randint(0, n_users, n_pairs), rs.randint(0, n_users, n)])
    sidx = np.concatenate([rs.choice(n, n_pairs, p=p / p.sum()), np.arange(n)])  # every song has a play
    split = np.arange(n, dtype=np.int64)
    indptr, ranks = user_split_ranks(uidx, sidx, n_users, split)
    counts = np.bincount(ranks, minlength=n)  # distinct users per song
    w = popularity_weights(counts, args.alpha)
    tables = weighted_split_tables(indptr, ranks, w)

    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    split_d, indptr_d, ranks_d = to(split), to(indptr), to(ranks)
    tab_d = [to(a.view(np.int32)) for a in tables]
    tab = nat.WeightTables(*[a.data_ptr() for a in tab_d])
    n_batches = args.inner * (args.reps + args.warmup)
    users_h = rs.randint(0, n_users, (n_batches, B)).astype(np.int64)
    users_d = to(users_h)
    out = torch.empty((B, N), dtype=torch.int64, device=dev)
    mt = torch.empty(nat.MT_STATE_BYTES, dtype=torch.uint8, device=dev)
    lib, stream = nat.lib(), nat.stream_handle(dev)

    def weighted(k, reseed=0):
        nat.check(lib.dcue_sample_catalogue_weighted(
            None if reseed else nat.ptr(mt), reseed, 1234, nat.ptr(split_d), n, nat.ptr(indptr_d), nat.ptr(ranks_d),
            ctypes.byref(tab), nat.ptr(users_d[k]), B, N, nat.ptr(out), stream), "dcue_sample_catalogue_weighted")

    def uniform(k):
        nat.check(lib.dcue_sample_catalogue(nat.ptr(mt), 0, 0, nat.ptr(split_d), n, nat.ptr(indptr_d), nat.ptr(ranks_d),
                                            nat.ptr(users_d[k]), B, N, nat.ptr(out), stream), "dcue_sample_catalogue")

    # agreement with the definition on the first batch
    nat.check(lib.dcue_mt_seed(nat.ptr(mt), 77, stream), "dcue_mt_seed")
    weighted(0)
    same = bool(np.array_equal(out.cpu().numpy(), R.sample_users(77, False, split, w, indptr, ranks, users_h[0], N)))
    print("agreement: the first batch equals the numpy definition: %s" % same, file=sys.stderr)
    assert same

    routes = {"weighted_stream": weighted, "uniform_stream": uniform, "weighted_reseed": lambda k: weighted(k, 1)}
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

    ms = {name: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for name, v in times.items()}
    step = args.step_ms
    res = {
        "bench": "weighted_sampler", "device": torch.cuda.get_device_name(0),
        "shape": {"split_songs": n, "users": n_users, "mean_split_plays_per_user": float(len(ranks)) / n_users,
                  "samples": B, "neg": N, "alpha": args.alpha, "total_weight": int(tables[0][-1]),
                  "max_weight": int(w.max()), "min_weight": int(w.min())},
        "reps": args.reps, "inner": args.inner, "warmup": args.warmup,
        "ms_per_call": ms,
        "weighted_over_uniform": ms["weighted_stream"]["median"] / ms["uniform_stream"]["median"],
        "parent_catalogue_step_ms": step, "parent_catalogue_step_source": args.step_source if step is not None else None,
        # the condition: the slowest weighted draw seen stays below one training step
        "weighted_draw_below_one_step": None if step is None else bool(ms["weighted_stream"]["max"] < step),
        "agreement_bitwise": same,
        "not_measured": ["the kernels alone without their launches (rocprofv3)", "other N and batch sizes",
                         "users with thousands of plays (lists past the LDS stage)",
                         "total weights near 2^32", "a real sub-epoch's wall time", "ranking quality"],
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
