#!/usr/bin/env python
"""Turn a directory of wave files into the log-mel spectrograms and the metadata CSV the datasets read.

The reference's README names a transform_audio.py that was never published; this is that step for the
MI355X build, on the GPU (dcrecommend.audio.LogMel, include/dcue.h dcue_logmel):

  python transform_audio.py --wav-dir clips/ --out-dir mels/ --metadata metadata.csv
  python transform_audio.py ... --n-fft 2048 --hop 512 --compress log1p --top-db 80
  python transform_audio.py ... --resample best      # 44.1 / 48 kHz files in, 22,050 Hz spectrograms out

Every *.wav under --wav-dir (16-bit PCM, mono or stereo) becomes one torch.save'd float32 [128, T] tensor
in --out-dir, T = 1 + n_samples // hop frames of the clip at --sample-rate. A file at another rate is an
error with --resample off (the default); with best or fast it is resampled on the GPU first
(dcrecommend.audio.Resampler, include/dcue.h dcue_resample). Files of equal rate and length go through
the GPU together, --batch at a time.
The CSV has the columns idx, song_id, data_mel -- song_id (the file's name without .wav) in column 1 and
the tensor's path in `data_mel`, as datasets/dcueitemset.py reads them. The item tower takes 131
frames: 66,560 samples (3.02 s) at the defaults.
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "amplifai-deepcontentrecommenders_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--wav-dir", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--metadata", required=True, help="CSV to write: idx, song_id, data_mel")
    ap.add_argument("--sample-rate", type=int, default=22050)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--fmin", type=float, default=0.0)
    ap.add_argument("--fmax", type=float, default=None)
    ap.add_argument("--compress", choices=["db", "log1p", "power"], default="db")
    ap.add_argument("--amin", type=float, default=1e-10)
    ap.add_argument("--log-scale", type=float, default=10.0)
    ap.add_argument("--top-db", type=float, default=None)
    ap.add_argument("--resample", choices=["off", "best", "fast"], default="off",
                    help="resample files at another rate on the GPU (off: such a file is an error)")
    ap.add_argument("--batch", type=int, default=256, help="clips of one rate and length per GPU call")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    from dcrecommend import audio
    names = sorted(f for f in os.listdir(args.wav_dir) if f.lower().endswith(".wav"))
    if not names:
        raise SystemExit("transform_audio: no .wav files in %s" % args.wav_dir)
    lm = audio.LogMel(sample_rate=args.sample_rate, n_fft=args.n_fft, hop=args.hop, fmin=args.fmin, fmax=args.fmax,
                      compress=args.compress, amin=args.amin, log_scale=args.log_scale, top_db=args.top_db,
                      device=args.device)
    os.makedirs(args.out_dir, exist_ok=True)
    by_length = {}
    for name in names:  # files of equal rate and length share a launch
        x, rate = audio.read_wav(os.path.join(args.wav_dir, name),
                                 sample_rate=args.sample_rate if args.resample == "off" else None)
        by_length.setdefault((rate, len(x)), []).append((name, x))
    paths = {}
    for (rate, length), clips in sorted(by_length.items()):
        for s in range(0, len(clips), args.batch):
            part = clips[s:s + args.batch]
            try:
                wave = np.stack([x for _, x in part])
                if rate == args.sample_rate:
                    mel = lm.reference_tensor(wave).cpu()
                else:
                    mel = lm.reference_tensor(wave, source_rate=rate, resample=args.resample).cpu()
            except ValueError as e:
                raise SystemExit("transform_audio: %s (%d-sample files %s ...)" % (e, length, part[0][0]))
            for (name, _), m in zip(part, mel):
                paths[name] = os.path.abspath(os.path.join(args.out_dir, name[:-4] + ".pt"))
                torch.save(m.clone(), paths[name])
    with open(args.metadata, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["idx", "song_id", "data_mel"])
        for i, name in enumerate(names):
            w.writerow([i, name[:-4], paths[name]])
    print("transform_audio: %d files, %d (rate, length) groups -> %s" % (len(names), len(by_length), args.metadata))
    return 0


if __name__ == "__main__":
    sys.exit(main())
