"""The audio front end: waveforms to the log-mel spectrograms the item tower reads, on the GPU in
one fused launch (include/dcue.h, dcue_logmel), sample-rate conversion ahead of it (dcue_resample), and
a reader for 16-bit PCM wave files.

The reference project names a transform_audio.py that was never published; the conventions here
(periodic Hann, reflect padding, Slaney mel scale with area normalisation, 10 log10 with a floor) are
librosa's defaults, stated in include/dcue.h and pinned by tests/logmel_reference.py."""
import ctypes
import wave as _wave

import numpy as np
import torch

from . import _native as nat


def _config(sample_rate, n_fft, hop, center, compress, out_dtype, fmin, fmax, amin, log_scale):
    return nat.LogmelConfig(int(sample_rate), int(n_fft), int(hop), int(bool(center)), int(compress), int(out_dtype),
                            float(fmin), float(fmax), float(amin), float(log_scale))


def _invalid_is_value_error(status, what):
    if status == 1:  # DCUE_ERR_INVALID: the library says which argument
        raise ValueError(nat.lib().dcue_last_error().decode(errors="replace"))
    nat.check(status, what)


class Resampler:
    """rate_in -> rate_out on the GPU (include/dcue.h, dcue_resample): a rational polyphase resampler with
    a Kaiser-windowed sinc evaluated exactly per phase. quality: "best", "fast" (nat.RESAMPLE_QUALITIES)
    or an explicit (zeros, beta, rolloff) triple. The constructor validates on the host (ValueError)
    before it touches the GPU. With equal rates resample() returns its input tensor as it is."""

    def __init__(self, rate_in, rate_out, quality="best", device="cuda"):
        if isinstance(quality, str):
            if quality not in nat.RESAMPLE_QUALITIES:
                raise ValueError("quality must be one of %s or a (zeros, beta, rolloff) triple, got %r"
                                 % (sorted(nat.RESAMPLE_QUALITIES), quality))
            quality = nat.RESAMPLE_QUALITIES[quality]
        try:
            zeros, beta, rolloff = quality
            zeros, beta, rolloff = int(zeros), float(beta), float(rolloff)
        except (TypeError, ValueError):
            raise ValueError("quality must be 'best', 'fast' or a (zeros, beta, rolloff) triple, got %r" % (quality,))
        self.rate_in, self.rate_out, self.quality = int(rate_in), int(rate_out), (zeros, beta, rolloff)
        self.device = torch.device(device)
        self._table, self._table_bytes = None, 0
        self.identity = self.rate_in == self.rate_out
        if self.identity:
            if self.rate_in < 1:
                raise ValueError("dcue_resample: rate_in and rate_out must be positive")
            return
        nbytes = ctypes.c_size_t()
        self._check(nat.lib().dcue_resample_table_bytes(ctypes.byref(self._cfg()), ctypes.byref(nbytes)),
                    "dcue_resample_table_bytes")
        self._table_bytes = nbytes.value

    _check = staticmethod(_invalid_is_value_error)

    def _cfg(self):
        return nat.ResampleConfig(self.rate_in, self.rate_out, self.quality[0], 0, self.quality[1], self.quality[2])

    def n_out(self, n_in):
        """Samples of an n_in-sample clip after conversion: ceil(n_in L / M)."""
        if self.identity:
            return int(n_in)
        n = ctypes.c_int64()
        self._check(nat.lib().dcue_resample_length(ctypes.byref(self._cfg()), int(n_in), ctypes.byref(n)),
                    "dcue_resample_length")
        return n.value

    def host_table(self):
        """The table's bytes as dcue_resample_table_fill_host computes them (uint8 numpy; no GPU)."""
        if self.identity:
            raise ValueError("dcue_resample: equal rates: nothing to resample")
        buf = np.zeros(self._table_bytes, dtype=np.uint8)
        self._check(nat.lib().dcue_resample_table_fill_host(ctypes.byref(self._cfg()), ctypes.c_void_p(buf.ctypes.data),
                                                            buf.nbytes), "dcue_resample_table_fill_host")
        return buf

    def _device_table(self):
        if self._table is None:
            table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)
            self._check(nat.lib().dcue_resample_table_init(ctypes.byref(self._cfg()), nat.ptr(table), table.numel(),
                                                           nat.stream_handle(self.device)), "dcue_resample_table_init")
            self._table = table
        return self._table

    def resample(self, wave, out0=0, n_out=None):
        """[n][n_out] float32 on the device: outputs out0 .. out0 + n_out - 1 (default: to the end) of
        each clip of wave ([n_in] or [n][n_in])."""
        if self.identity:
            if out0 != 0 or n_out is not None:
                raise ValueError("dcue_resample: equal rates: nothing to resample (slice the input instead)")
            return wave
        w = torch.as_tensor(wave)
        if w.dim() == 1:
            w = w.unsqueeze(0)
        if w.dim() != 2:
            raise ValueError("wave must be [n_samples] or [n_clips][n_samples], got shape %s" % (tuple(w.shape),))
        w = w.to(device=self.device, dtype=torch.float32).contiguous()
        n, n_in = int(w.shape[0]), int(w.shape[1])
        total = self.n_out(n_in)
        count = total - int(out0) if n_out is None else int(n_out)
        out = torch.empty((n, max(count, 0)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(nat.lib().dcue_resample(ctypes.byref(self._cfg()), nat.ptr(self._device_table()), nat.ptr(w), n,
                                                n_in, int(out0), count, nat.ptr(out), nat.stream_handle(self.device)),
                        "dcue_resample")
        return out


class LogMel:
    """One front-end configuration and its device table (window, twiddles, mel filters).

    compress: "db" (10 log10(max(P, amin))), "log1p" (log(1 + log_scale sqrt(P))) or "power".
    top_db (dB mode only): each clip is clamped at its own maximum minus top_db, on the output.
    The constructor validates the configuration on the host (ValueError) before it touches the GPU."""

    def __init__(self, sample_rate=22050, n_fft=1024, hop=512, fmin=0.0, fmax=None, compress="db", amin=1e-10,
                 log_scale=10.0, top_db=None, center=True, device="cuda"):
        if compress not in nat.LOGMEL_MODES:
            raise ValueError("compress must be one of %s, got %r" % (sorted(nat.LOGMEL_MODES), compress))
        if top_db is not None and (compress != "db" or not top_db >= 0):
            raise ValueError("top_db needs compress='db' and a value >= 0")
        self.sample_rate, self.n_fft, self.hop, self.center = int(sample_rate), int(n_fft), int(hop), bool(center)
        self.fmin, self.fmax = float(fmin), float(sample_rate) / 2.0 if fmax is None else float(fmax)
        self.compress, self.amin, self.log_scale, self.top_db = compress, float(amin), float(log_scale), top_db
        self.device = torch.device(device)
        nbytes = ctypes.c_size_t()
        self._check(nat.lib().dcue_logmel_table_bytes(ctypes.byref(self._cfg(torch.float32)), ctypes.byref(nbytes)),
                    "dcue_logmel_table_bytes")
        self._table_bytes = nbytes.value
        self._table = None
        self._resamplers = {}

    def _cfg(self, dtype):
        if dtype not in (torch.float16, torch.float32):
            raise ValueError("dtype must be torch.float16 or torch.float32, got %s" % dtype)
        return _config(self.sample_rate, self.n_fft, self.hop, self.center, nat.LOGMEL_MODES[self.compress],
                       0 if dtype == torch.float16 else 1, self.fmin, self.fmax, self.amin, self.log_scale)

    _check = staticmethod(_invalid_is_value_error)

    def host_table(self):
        """The table's bytes as dcue_logmel_table_fill_host computes them (uint8 numpy; no GPU)."""
        buf = np.zeros(self._table_bytes, dtype=np.uint8)
        self._check(nat.lib().dcue_logmel_table_fill_host(ctypes.byref(self._cfg(torch.float32)),
                                                          ctypes.c_void_p(buf.ctypes.data), buf.nbytes),
                    "dcue_logmel_table_fill_host")
        return buf

    def _device_table(self):
        if self._table is None:
            table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)
            self._check(nat.lib().dcue_logmel_table_init(ctypes.byref(self._cfg(torch.float32)), nat.ptr(table),
                                                         table.numel(), nat.stream_handle(self.device)),
                        "dcue_logmel_table_init")
            self._table = table
        return self._table

    def n_frames(self, n_samples):
        """Frames of an n_samples clip: 1 + (n_samples + 2 pad - n_fft) // hop."""
        n = ctypes.c_int64()
        self._check(nat.lib().dcue_logmel_frames(ctypes.byref(self._cfg(torch.float32)), int(n_samples),
                                                 ctypes.byref(n)), "dcue_logmel_frames")
        return n.value

    def _wave(self, wave):
        w = torch.as_tensor(wave)
        if w.dim() == 1:
            w = w.unsqueeze(0)
        if w.dim() != 2:
            raise ValueError("wave must be [n_samples] or [n_clips][n_samples], got shape %s" % (tuple(w.shape),))
        return w.to(device=self.device, dtype=torch.float32).contiguous()

    def resampler(self, source_rate, quality="best"):
        """The audio.Resampler from source_rate to this front end's rate, kept per (rate, quality)."""
        key = (int(source_rate), quality if isinstance(quality, str) else tuple(quality))
        if key not in self._resamplers:
            self._resamplers[key] = Resampler(int(source_rate), self.sample_rate, quality, self.device)
        return self._resamplers[key]

    def _at_rate(self, wave, source_rate, resample):
        if source_rate is None or int(source_rate) == self.sample_rate:
            return wave
        return self.resampler(source_rate, resample).resample(wave)

    def transform_raw(self, wave, frame0=0, n_frames=None, dtype=torch.float32, source_rate=None, resample="best"):
        """(out [n][T][128] of dtype, flags int32 [n]) device tensors as dcue_logmel writes them: no
        flag check and no top_db. source_rate: the rate of `wave` when it is not sample_rate -- the clips
        are resampled first (audio.Resampler, quality `resample`), and frame0 / n_frames count frames of
        the resampled clip."""
        w = self._wave(self._at_rate(wave, source_rate, resample))
        n, n_samples = int(w.shape[0]), int(w.shape[1])
        cfg = self._cfg(dtype)
        total = self.n_frames(n_samples)
        T = total - int(frame0) if n_frames is None else int(n_frames)
        out = torch.empty((n, max(T, 0), nat.N_MELS), dtype=dtype, device=self.device)
        flags = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(nat.lib().dcue_logmel(ctypes.byref(cfg), nat.ptr(self._device_table()), nat.ptr(w), n, n_samples,
                                              int(frame0), T, nat.ptr(out), nat.ptr(flags),
                                              nat.stream_handle(self.device)), "dcue_logmel")
        return out, flags[:n]

    def transform(self, wave, frame0=0, n_frames=None, dtype=torch.float32, source_rate=None, resample="best"):
        """[n][T][128] log-mel rows (frame-major: the track-table layout) of frames frame0 ..
        frame0 + n_frames - 1 (default: to the clip's last frame). Raises ValueError naming the clips
        that hold a NaN or infinite sample. source_rate / resample: as transform_raw."""
        out, flags = self.transform_raw(wave, frame0, n_frames, dtype, source_rate, resample)
        bad = torch.nonzero(flags & nat.LOGMEL_FLAG_NONFINITE).flatten().tolist()
        if bad:
            raise ValueError("non-finite samples in clip%s %s" % ("s" if len(bad) > 1 else "",
                                                                  ", ".join(str(b) for b in bad)))
        if self.top_db is not None and out.numel():
            f = out.float()
            out = torch.maximum(f, torch.amax(f, dim=(1, 2), keepdim=True) - float(self.top_db)).to(dtype)
        return out

    def track_rows(self, wave, frame0=0, dtype=torch.float16, source_rate=None, resample="best"):
        """[n][131][128]: a track table (dcue_tracks.data) of the clips' 131 frames from frame0."""
        return self.transform(wave, frame0, nat.N_FRAMES, dtype, source_rate, resample)

    def reference_tensor(self, wave, source_rate=None, resample="best"):
        """[n][128][T] float32: the layout of the reference's data_mel files."""
        return self.transform(wave, source_rate=source_rate, resample=resample).transpose(1, 2).contiguous()


def read_wav(path, sample_rate=None):
    """(float32 mono samples in [-1, 1), sample rate) of a 16-bit PCM wave file; stereo (any channel
    count) is averaged to mono. Other sample widths are refused, and so is a rate that differs from
    `sample_rate` when one is given: this reader does not resample (audio.Resampler and LogMel's
    source_rate do, on the GPU)."""
    with _wave.open(str(path), "rb") as f:
        width, channels, rate, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
        if width != 2:
            raise ValueError("%s: %d-bit samples; only 16-bit PCM is read" % (path, 8 * width))
        if f.getcomptype() != "NONE":
            raise ValueError("%s: compressed wave files are not read" % path)
        raw = f.readframes(n)
    if sample_rate is not None and rate != int(sample_rate):
        raise ValueError("%s: sample rate %d, configured %d (resample first)" % (path, rate, int(sample_rate)))
    x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    x = x.reshape(-1, channels)
    return (x[:, 0] if channels == 1 else x.mean(axis=1, dtype=np.float32)).copy(), rate
