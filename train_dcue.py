#!/usr/bin/env python
"""Train DCUE on MI355X through the reference's trainer API (dcrecommend.nn.dcue.DCUE).

The reference's README describes train_*.py drivers that build the datasets and call the trainer;
this is that driver for the MI355X build:

  python train_dcue.py --triplets triplets.csv --metadata metadata.csv --save-dir models/
  python train_dcue.py --synthetic --num-epochs 1 --save-dir /tmp/dcue   # self-contained demo
  python train_dcue.py ... --recommend-k 10 --recommend-out recs.csv      # + each user's top 10
  python train_dcue.py ... --recommend-k 10 --recommend-out recs.csv --recommend-for new.csv
                                                  # the top 10 of users outside the training set
  python train_dcue.py ... --eval-k 10,50,100 --eval-out metrics.json     # + top-K ranking metrics
  python train_dcue.py ... --recommend-k 10 --recommend-out recs.csv --recommend-diversity 0.7
                                                  # MMR re-ranked lists (--recommend-pool: the pool)
  python train_dcue.py ... --recommend-k 10 --recommend-out recs.csv --recommend-reasons 3 --reasons-out why.csv
                                                  # + each pick's 3 nearest songs of the user's history
  python train_dcue.py ... --artists artists.csv --recommend-k 10 --recommend-out recs.csv --recommend-max-per-artist 2
                                                  # at most two songs per artist (--recommend-new-artists:
                                                  # none by an artist the user has played)
  python train_dcue.py ... --artists artists.csv --recommend-k 10 --recommend-out recs.csv --recommend-artists-out a.csv
                                                  # + each user's 10 best artists
  python train_dcue.py ... --eval-k 10,50 --eval-out metrics.json --eval-ild --eval-diversity 0.7
  python train_dcue.py ... --recommend-k 10 --recommend-out recs.csv --recommend-popularity -0.2
                                                  # demote the hits (--popularity counts.csv: whose counts)
  python train_dcue.py ... --eval-k 10,50 --eval-out metrics.json --eval-novelty --eval-popularity -0.2
                                                  # + novelty@K, tail@K, gini@K of the demoted lists
                                                  # + intra-list diversity, of the MMR re-ranked lists

triplets: (user_id, song_id, score) by column position (datasets/dcuedataset.py:229,238);
metadata: song_id in column 1 and a `data_mel` column of torch.save'd [128, T] tensors
(datasets/dcueitemset.py:46,50). Arguments mirror DCUE's constructor (nn/dcue.py:47-50).
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--triplets")
    ap.add_argument("--metadata")
    ap.add_argument("--save-dir", default="models")
    ap.add_argument("--synthetic", action="store_true",
                    help="generate a small synthetic interaction set and spectrogram files")
    ap.add_argument("--synthetic-users", type=int, default=60)
    ap.add_argument("--synthetic-tracks", type=int, default=120)
    ap.add_argument("--synthetic-pairs", type=int, default=1500)
    ap.add_argument("--feature-dim", type=int, default=100)  # DCUE's default, nn/dcue.py:44
    ap.add_argument("--conv-hidden", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--neg-batch-size", type=int, default=20)
    ap.add_argument("--u-embdim", type=int, default=300)
    ap.add_argument("--margin", type=float, default=0.2)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--optimize", choices=["adam", "sgd", "ranger"], default="adam",
                    help="DCUE(optimize=...): nn/dcue.py:143-157")
    ap.add_argument("--model-type", default="truedcuemel1dbn", help="DCUE(model_type=...): dcue/dcue.py:49-59")
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--num-epochs", type=int, default=90)
    ap.add_argument("--eval-pct", type=float, default=0.025)
    ap.add_argument("--val-pct", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--recommend-k", type=int, default=0,
                    help="after training, the K best unseen songs of every training user (0: off)")
    ap.add_argument("--recommend-out", help="CSV for --recommend-k: user_id, rank, song_id, score")
    ap.add_argument("--recommend-for", metavar="FILE.csv",
                    help="columns user_id,song_id: histories of users outside the training set; their "
                         "lists (DCUE.recommend_for: fold-in, then top K) are written instead of the "
                         "training users'")
    ap.add_argument("--recommend-diversity", type=float, metavar="L",
                    help="MMR re-ranking of the --recommend-k / --recommend-for lists with lambda = L in [0, 1] "
                         "(DCUE.recommend(diversity=L)); default: the plain ranking")
    ap.add_argument("--recommend-pool", type=int, metavar="P",
                    help="candidates ranked per user before the MMR pass (K..128; default min(128, 4 K))")
    ap.add_argument("--recommend-reasons", type=int, metavar="M",
                    help="with --recommend-k: for every pick the M (1..8) songs of the user's history nearest to "
                         "it by the item factors' cosine (DCUE.explain / explain_for), written to --reasons-out")
    ap.add_argument("--reasons-out", help="CSV for --recommend-reasons: user_id, rank, song_id, reason_rank, "
                                          "reason_song_id, similarity")
    ap.add_argument("--artists", metavar="FILE.csv",
                    help="columns song_id,artist: who recorded each song (DCUE.set_artists); songs it leaves out "
                         "have no artist and are never capped")
    ap.add_argument("--recommend-max-per-artist", type=int, metavar="M",
                    help="with --artists: no artist holds more than M songs of a --recommend-k / --recommend-for "
                         "list (DCUE.recommend(max_per_artist=M)); --recommend-pool sets the pool here too")
    ap.add_argument("--recommend-new-artists", action="store_true",
                    help="with --artists: the lists leave out every song by an artist the user has played")
    ap.add_argument("--recommend-artists-out", metavar="FILE.csv",
                    help="with --artists and --recommend-k: each training user's K best artists "
                         "(DCUE.recommend_artists): user_id, rank, artist, song_id, score")
    ap.add_argument("--eval-artists", action="store_true",
                    help="with --artists: --eval-k also reports artists@K, artist_top@K and artist_coverage@K, and "
                         "scores the --recommend-max-per-artist lists when that is set")
    ap.add_argument("--eval-k", metavar="K[,K...]",
                    help="after training, Precision / Recall / NDCG / MAP / MRR / HitRate / coverage at these "
                         "cutoffs over the val and the test split (DCUE.evaluate_topk)")
    ap.add_argument("--eval-out", help="JSON for --eval-k: {\"val\": {...}, \"test\": {...}}")
    ap.add_argument("--eval-ild", action="store_true",
                    help="--eval-k also reports ild@K, the lists' mean intra-list diversity")
    ap.add_argument("--eval-diversity", type=float, metavar="L",
                    help="--eval-k scores the MMR re-ranked lists (lambda = L) instead of the plain ranking")
    ap.add_argument("--popularity", metavar="FILE.csv",
                    help="song_id, count: the play counts behind --recommend-popularity / --eval-popularity / "
                         "--eval-novelty (DCUE.set_popularity); default: the training data's per-song user counts")
    ap.add_argument("--recommend-popularity", type=float, metavar="B",
                    help="the --recommend-k / --recommend-for lists rank by cosine + B * (the song's scaled "
                         "log-popularity in [0, 1]): B < 0 demotes the hits, B > 0 promotes them "
                         "(DCUE.recommend(popularity=B)); default: the plain ranking")
    ap.add_argument("--eval-popularity", type=float, metavar="B",
                    help="--eval-k scores the lists --recommend-popularity B would serve")
    ap.add_argument("--eval-novelty", action="store_true",
                    help="--eval-k also reports novelty@K, tail@K and gini@K")
    ap.add_argument("--crop", choices=["load", "epoch"], default="load",
                    help="DCUE(crop=...): 'load' cuts each track's 131-frame window once, when the catalogue is "
                         "loaded; 'epoch' keeps the full-length tracks in HBM and cuts a fresh random window of "
                         "every track before each training sub-epoch (dcue_crop_tracks)")
    ap.add_argument("--crop-seed", type=int, default=0, help="DCUE(crop_seed=...): the seed of --crop epoch's windows")
    ap.add_argument("--factor-crops", choices=["random", "grid"], default="random",
                    help="DCUE(factor_crops=...), with --crop epoch: the windows the item factors average over")
    ap.add_argument("--neg-sampling", choices=["uniform", "popularity"], default="uniform",
                    help="DCUEDataset(neg_sampling=...) of the TRAIN set: 'popularity' draws a user's negatives in "
                         "proportion to (a song's number of users) ** --neg-alpha instead of uniformly. The val and "
                         "test sets keep uniform negatives, so their losses stay comparable across runs")
    ap.add_argument("--neg-alpha", type=float, default=0.75, help="the exponent of --neg-sampling popularity")
    ap.add_argument("--neg-pool", type=int, metavar="P",
                    help="DCUE(neg_pool=...): hard negatives for the training sub-epochs. Every row draws P "
                         "candidates (--neg-batch-size <= P <= 1024) and keeps the --neg-hard that the last "
                         "sub-epoch's factors score highest for its user, filled up with the other draws in order "
                         "(dcue_select_negatives). Default: the plain sampler. Val and test losses keep plain draws")
    ap.add_argument("--neg-hard", type=int, metavar="H",
                    help="DCUE(neg_hard=...), with --neg-pool: hard negatives per row, 0 <= H <= --neg-batch-size "
                         "(default: half of --neg-batch-size)")
    ap.add_argument("--augment-freq-masks", type=int, metavar="N",
                    help="DCUE(augment=...), with --crop epoch: frequency masks per track (0..4) applied while the "
                         "training table is re-cut (dcue_crop_tracks_augmented); val losses and factors stay clean")
    ap.add_argument("--augment-freq-width", type=int, metavar="F", help="largest width of a frequency mask, in mel bins (0..128)")
    ap.add_argument("--augment-time-masks", type=int, metavar="N", help="time masks per track (0..4)")
    ap.add_argument("--augment-time-width", type=int, metavar="T", help="largest width of a time mask, in frames (0..131)")
    ap.add_argument("--augment-gain-db", type=float, metavar="G",
                    help="loudness jitter: every track's window is shifted by a gain drawn from [-G, G)")
    ap.add_argument("--augment-fill", type=_augment_fill, metavar="{mean,<float>}",
                    help="what a masked element becomes: the window's mean (default) or a constant")
    args = ap.parse_args(argv)
    if augment_of(args) is not None and args.crop != "epoch":
        ap.error("--augment-* need --crop epoch")
    if args.neg_alpha < 0:
        ap.error("--neg-alpha must be >= 0, got %r" % args.neg_alpha)
    if args.neg_hard is not None and args.neg_pool is None:
        ap.error("--neg-hard needs --neg-pool")
    if args.neg_pool is not None and not args.neg_batch_size <= args.neg_pool <= 1024:
        ap.error("--neg-pool must be in --neg-batch-size..1024, got %r" % args.neg_pool)
    if args.neg_hard is not None and not 0 <= args.neg_hard <= args.neg_batch_size:
        ap.error("--neg-hard must be in 0..--neg-batch-size, got %r" % args.neg_hard)
    if bool(args.eval_k) != bool(args.eval_out):
        ap.error("--eval-k and --eval-out go together")
    if args.eval_k:
        try:
            args.eval_k = [int(k) for k in args.eval_k.split(",")]
        except ValueError:
            ap.error("--eval-k takes comma-separated integers, got %r" % args.eval_k)
    if (args.recommend_k > 0) != bool(args.recommend_out):
        ap.error("--recommend-k and --recommend-out go together")
    if args.recommend_for and not args.recommend_out:
        ap.error("--recommend-for needs --recommend-k and --recommend-out")
    if (args.recommend_diversity is not None or args.recommend_pool is not None) and args.recommend_k <= 0:
        ap.error("--recommend-diversity / --recommend-pool need --recommend-k")
    if (args.recommend_pool is not None and args.recommend_diversity is None
            and args.recommend_max_per_artist is None):
        ap.error("--recommend-pool needs --recommend-diversity")
    artist_flags = [("--recommend-max-per-artist", args.recommend_max_per_artist is not None),
                    ("--recommend-new-artists", args.recommend_new_artists),
                    ("--recommend-artists-out", bool(args.recommend_artists_out)), ("--eval-artists", args.eval_artists)]
    for flag, given in artist_flags:
        if given and not args.artists:
            ap.error("%s needs --artists" % flag)
    if any(given for _, given in artist_flags[:3]) and args.recommend_k <= 0:
        ap.error("--recommend-max-per-artist / --recommend-new-artists / --recommend-artists-out need --recommend-k")
    if args.recommend_max_per_artist is not None and args.recommend_max_per_artist < 1:
        ap.error("--recommend-max-per-artist must be at least 1, got %r" % args.recommend_max_per_artist)
    if args.recommend_artists_out and args.recommend_for:
        ap.error("--recommend-artists-out goes without --recommend-for")
    if args.eval_artists and not args.eval_k:
        ap.error("--eval-artists needs --eval-k")
    if (args.recommend_reasons is not None) != bool(args.reasons_out):
        ap.error("--recommend-reasons and --reasons-out go together")
    if args.recommend_reasons is not None and args.recommend_k <= 0:
        ap.error("--recommend-reasons / --reasons-out need --recommend-k")
    if args.recommend_reasons is not None and not 1 <= args.recommend_reasons <= 8:
        ap.error("--recommend-reasons must be in 1..8, got %r" % args.recommend_reasons)
    if (args.eval_ild or args.eval_diversity is not None) and not args.eval_k:
        ap.error("--eval-ild / --eval-diversity need --eval-k")
    if args.recommend_popularity is not None and args.recommend_k <= 0:
        ap.error("--recommend-popularity needs --recommend-k")
    if (args.eval_popularity is not None or args.eval_novelty) and not args.eval_k:
        ap.error("--eval-popularity / --eval-novelty need --eval-k")
    if args.popularity and args.recommend_popularity is None and args.eval_popularity is None and not args.eval_novelty:
        ap.error("--popularity goes with --recommend-popularity, --eval-popularity or --eval-novelty")
    for name in ("recommend_popularity", "eval_popularity"):
        if getattr(args, name) is not None and not np.isfinite(getattr(args, name)):
            ap.error("--%s takes a finite number, got %r" % (name.replace("_", "-"), getattr(args, name)))
    for name in ("recommend_diversity", "eval_diversity"):
        lam = getattr(args, name)
        if lam is not None and not 0.0 <= lam <= 1.0:
            ap.error("--%s takes a lambda in [0, 1], got %r" % (name.replace("_", "-"), lam))
    return args


def _augment_fill(text):
    if text == "mean":
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("'mean' or a number, got %r" % text)


def augment_of(args):
    """The --augment-* options that were given, as DCUE(augment=...) takes them; None when none was."""
    names = ("freq_masks", "freq_width", "time_masks", "time_width", "gain_db", "fill")
    given = {n: getattr(args, "augment_" + n) for n in names if getattr(args, "augment_" + n) is not None}
    return given or None


def synthetic_data(n_users, n_tracks, n_pairs, out_dir, seed):
    """Unique (user, song) pairs and fp16-representable 131-frame spectrograms on disk."""
    rs = np.random.RandomState(seed)
    pairs = set()
    while len(pairs) < n_pairs:
        pairs.add((int(rs.randint(n_users)), int(rs.randint(n_tracks))))
    pairs = sorted(pairs)
    trip = pd.DataFrame({"user_id": ["u%06d" % u for u, _ in pairs],
                         "song_id": ["S%07d" % s for _, s in pairs],
                         "score": rs.randint(1, 10, size=len(pairs))})
    songs = sorted(set(trip["song_id"]))
    gen = torch.Generator().manual_seed(seed)
    paths = []
    for k, _ in enumerate(songs):
        p = os.path.join(out_dir, "mel_%06d.pt" % k)
        torch.save(torch.randn(128, 131, generator=gen).half().float(), p)
        paths.append(p)
    meta = pd.DataFrame({"idx": np.arange(len(songs)), "song_id": songs, "data_mel": paths})
    return trip, meta


def main(argv=None):
    args = parse(argv)
    from dcrecommend.datasets.dcuedataset import DCUEDataset
    from dcrecommend.datasets.dcueitemset import DCUEItemset
    from dcrecommend.datasets.dcuepredset import DCUEPredset
    from dcrecommend.nn.dcue import DCUE

    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.synthetic:
        mel_dir = tempfile.mkdtemp(prefix="dcue_mel_")
        trip, meta = synthetic_data(args.synthetic_users, args.synthetic_tracks, args.synthetic_pairs,
                                    mel_dir, args.seed)
        triplets_path, metadata_path = "<synthetic>", mel_dir
    else:
        if not args.triplets or not args.metadata:
            raise SystemExit("--triplets and --metadata are required (or --synthetic)")
        trip = pd.read_csv(args.triplets)
        meta = pd.read_csv(args.metadata)
        triplets_path, metadata_path = args.triplets, args.metadata

    train = DCUEDataset(trip.copy(), meta, neg_samples=args.neg_batch_size, split="train",
                        neg_sampling=args.neg_sampling, neg_alpha=args.neg_alpha)
    val = DCUEDataset(trip.copy(), meta, neg_samples=args.neg_batch_size, split="val")
    test = DCUEDataset(trip.copy(), meta, neg_samples=args.neg_batch_size, split="test")
    pred = DCUEPredset(trip.copy(), meta, split="val")
    truth = DCUEPredset(trip.copy(), meta, split="train")
    items = DCUEItemset(trip.copy(), meta)
    dcue = DCUE(feature_dim=args.feature_dim, conv_hidden=args.conv_hidden, batch_size=args.batch_size,
                neg_batch_size=args.neg_batch_size, u_embdim=args.u_embdim, margin=args.margin, lr=args.lr,
                weight_decay=args.weight_decay, num_epochs=args.num_epochs, eval_pct=args.eval_pct,
                val_pct=args.val_pct, optimize=args.optimize, model_type=args.model_type, crop=args.crop,
                crop_seed=args.crop_seed, factor_crops=args.factor_crops, neg_pool=args.neg_pool,
                neg_hard=args.neg_hard, augment=augment_of(args))
    dcue.fit(train, val, test, pred, truth, items, len(train.user_index), len(train.item_index),
             triplets_path, metadata_path, args.save_dir)
    artist_kw = {}
    if args.artists:
        names = pd.read_csv(args.artists, dtype=str)
        dcue.set_artists(dict(zip(names["song_id"], names["artist"])))
        artist_kw = dict(max_per_artist=args.recommend_max_per_artist, new_artists=args.recommend_new_artists)
    if args.recommend_popularity is not None or args.eval_popularity is not None or args.eval_novelty:
        counts = None
        if args.popularity:
            table = pd.read_csv(args.popularity, dtype={"song_id": str})
            counts = {s: int(c) for s, c in zip(table["song_id"], table["count"])}
        dcue.set_popularity(counts)
    if args.recommend_popularity is not None:
        artist_kw = dict(artist_kw, popularity=args.recommend_popularity)
    if args.recommend_k > 0 and args.recommend_out:
        if args.recommend_for:
            new = pd.read_csv(args.recommend_for, dtype=str)
            histories = {u: list(g) for u, g in new.groupby("user_id", sort=False)["song_id"]}
            write_recommendations(dcue, list(histories), args.recommend_k, args.recommend_out,
                                  histories=histories, seed=args.seed, diversity=args.recommend_diversity,
                                  pool=args.recommend_pool, reasons=args.recommend_reasons,
                                  reasons_path=args.reasons_out, **artist_kw)
        else:
            write_recommendations(dcue, list(train.uniq_users), args.recommend_k, args.recommend_out,
                                  diversity=args.recommend_diversity, pool=args.recommend_pool,
                                  reasons=args.recommend_reasons, reasons_path=args.reasons_out, **artist_kw)
        if args.recommend_artists_out:
            write_artists(dcue, list(train.uniq_users), args.recommend_k, args.recommend_artists_out,
                          new_artists=args.recommend_new_artists, popularity=args.recommend_popularity)
    if args.eval_k:
        write_metrics(dcue, val, test, args.eval_k, args.eval_out, diversity=args.eval_diversity, ild=args.eval_ild,
                      artists=args.eval_artists, max_per_artist=args.recommend_max_per_artist if args.eval_artists else None,
                      popularity=args.eval_popularity, novelty=args.eval_novelty)
    return dcue


def write_artists(dcue, users, k, path, new_artists=False, popularity=None):
    """The best-by-validation factors' k best artists per user (DCUE.recommend_artists), one CSV row per
    (user, rank): the artist, and the song of theirs that ranks highest for the user with its score."""
    if dcue.best_user_factors is not None:
        dcue.insert_best_factors()
    pkw = {} if popularity is None else dict(popularity=popularity)
    lists = dcue.recommend_artists(users, k=k, new_artists=new_artists, **pkw)
    rows = [(u, r + 1, artist, song, score) for u, lst in zip(users, lists) for r, (artist, song, score) in enumerate(lst)]
    pd.DataFrame(rows, columns=["user_id", "rank", "artist", "song_id", "score"]).to_csv(path, index=False)


def write_metrics(dcue, val, test, ks, path, diversity=None, ild=False, artists=False, max_per_artist=None,
                  popularity=None, novelty=False):
    """The best-by-validation factors' top-K ranking metrics over the val and the test split's songs
    (diversity: of the MMR re-ranked lists; ild: with their intra-list diversity; artists: with the
    artist numbers; max_per_artist: of the capped lists; popularity: of the lists that prior serves; novelty:
    with novelty@K, tail@K and gini@K)."""
    if dcue.best_user_factors is not None:
        dcue.insert_best_factors()
    kw = dict(artists=True, max_per_artist=max_per_artist) if artists else {}
    if popularity is not None:
        kw["popularity"] = popularity
    if novelty:
        kw["novelty"] = True
    res = {"val": dcue.evaluate_topk(val, ks=ks, diversity=diversity, ild=ild, **kw),
           "test": dcue.evaluate_topk(test, ks=ks, diversity=diversity, ild=ild, **kw)}
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def write_recommendations(dcue, users, k, path, histories=None, seed=0, diversity=None, pool=None, reasons=None,
                          reasons_path=None, max_per_artist=None, new_artists=False, popularity=None):
    """The best-by-validation factors' top-k unseen songs per user, one CSV row per (user, rank).
    histories: {user_id: [song_id, ...]} of users outside the training set (DCUE.recommend_for).
    diversity / pool: MMR re-ranked lists (DCUE.recommend). reasons / reasons_path: also each pick's
    `reasons` nearest history songs (DCUE.explain / explain_for), one row per (user, rank, reason_rank).
    max_per_artist / new_artists / popularity: as DCUE.recommend (none given: today's calls)."""
    if dcue.best_user_factors is not None:
        dcue.insert_best_factors()
    akw = {}
    if max_per_artist is not None or new_artists:
        akw = dict(max_per_artist=max_per_artist, new_artists=new_artists)
    if popularity is not None:
        akw["popularity"] = popularity
    if reasons is not None:
        if histories is not None:
            lists = dcue.explain_for([histories[u] for u in users], k=k, reasons=reasons, seed=seed,
                                     diversity=diversity, pool=pool, **akw)
        else:
            lists = dcue.explain(users, k=k, reasons=reasons, diversity=diversity, pool=pool, **akw)
        why = [(u, r + 1, song, j + 1, h, sim) for u, lst in zip(users, lists)
               for r, (song, _, because) in enumerate(lst) for j, (h, sim) in enumerate(because)]
        pd.DataFrame(why, columns=["user_id", "rank", "song_id", "reason_rank", "reason_song_id",
                                   "similarity"]).to_csv(reasons_path, index=False)
        lists = [[(song, score) for song, score, _ in lst] for lst in lists]
    elif histories is not None:
        lists = dcue.recommend_for([histories[u] for u in users], k=k, seed=seed, diversity=diversity, pool=pool,
                                   **akw)
    else:
        lists = dcue.recommend(users, k=k, diversity=diversity, pool=pool, **akw)
    rows = [(u, r + 1, song, score) for u, lst in zip(users, lists) for r, (song, score) in enumerate(lst)]
    pd.DataFrame(rows, columns=["user_id", "rank", "song_id", "score"]).to_csv(path, index=False)


if __name__ == "__main__":
    main()
