"""Noisy mixtures on the device: the mixing of the reference's scripts/create_test_set.py:89-125 (process_save_utt: peak-normalise
the speech, scale a segment of a long noise recording to a target SNR, divide speech, noise and mixture by their common peak) for a
ragged batch of utterances in five launches (include/dvae.h: dvae_mix_snr_batch), the first stage of mix -> stft -> MCEM -> Wiener ->
istft -> score.  The outputs stay on the device, laid out for stft_packed if asked, and the noise comes back at the mixture's scale,
which is what energy_ratios_batch and McemBatch.score(s, n) need for SI-SIR and SI-SAR.  No CPU arithmetic exists here: without the
library or a GPU mix_at_snr_batch raises; mix_tables, condition_grid and draw_noise_starts are host logic and need neither.
"""
import numpy as np
import torch

from . import native as N
from . import ragged as R
from . import stft as H

MIX_CHUNK = 4096           # samples per work item (DVAE_MIX_CHUNK): fixed, so an utterance's sums never depend on the rest of the batch
STATS = ("p", "Ps", "Pn", "k", "norm", "snr_db")             # the columns of the [U, 6] stats


def _per_utterance(name, a, U):
    a = np.asarray(a).reshape(-1)
    if a.size != U:
        raise ValueError(f"mix_at_snr_batch: {name} has {a.size} entries for {U} utterances")
    return a


def mix_tables(speech_view, noise_view, starts, lengths, totals, out_layout=None):
    """The int64 table of dvae_mix_snr_batch, [items (U + 1) | speech0 (U) | noise0 (U) | out0 (U) | len (U) | out_extent (U)].

    speech_view: (offsets, lengths) of the U utterances inside the packed speech buffer; ranges may repeat (one utterance under many
    noises or SNRs).  noise_view: (bank_offsets, bank_lengths, noise_index): the banks inside the packed noise buffer and the bank of
    each utterance.  starts: the first sample of each utterance's noise segment inside its bank.  lengths: the samples to mix of each
    utterance, or None for the whole of it (a shorter length mixes the utterance's head).  totals: the element counts of the speech
    and noise buffers, and of the output buffers when out_layout is given.  out_layout: None (the outputs packed end to end at
    multiples of 64 samples, out_extent = len) or (out0, out_extent).

    ValueError naming the utterance for per-utterance lists whose lengths disagree, a speech range outside its buffer, a bank index
    that names no bank, a noise segment that leaves its bank, an out_extent shorter than the length, and output ranges that overlap or
    leave their buffer."""
    s_off, s_len = (np.asarray(a, np.int64).reshape(-1) for a in speech_view)
    U = s_off.size
    if U == 0:
        raise ValueError("mix_at_snr_batch: no utterances")
    if len(noise_view) != 3 or len(totals) < (2 if out_layout is None else 3):
        raise ValueError("mix_at_snr_batch: noise_view = (bank offsets, bank lengths, noise_index), and the element count of each buffer")
    b_off, b_len = (np.asarray(a, np.int64).reshape(-1) for a in noise_view[:2])
    if b_off.size == 0 or b_off.size != b_len.size:
        raise ValueError(f"mix_at_snr_batch: {b_off.size} bank offsets for {b_len.size} bank lengths")
    s_len = _per_utterance("the speech lengths", s_len, U).astype(np.int64)
    index = _per_utterance("noise_index", noise_view[2], U).astype(np.int64)
    starts = _per_utterance("starts", starts, U).astype(np.int64)
    length = s_len if lengths is None else _per_utterance("lengths", lengths, U).astype(np.int64)

    def first(mask):
        bad = np.flatnonzero(mask)
        return int(bad[0]) if bad.size else None

    u = first((length < 1) | (length > s_len))
    if u is not None:
        raise ValueError(f"mix_at_snr_batch: utterance {u} mixes {int(length[u])} samples of {int(s_len[u])}: at least one, at most all, is needed")
    u = first((s_off < 0) | (s_off + length > int(totals[0])))
    if u is not None:
        raise ValueError(f"mix_at_snr_batch: utterance {u} of speech ([{int(s_off[u])}, {int(s_off[u] + length[u])})) leaves its buffer "
                         f"({int(totals[0])} elements)")
    u = first((index < 0) | (index >= b_off.size))
    if u is not None:
        raise ValueError(f"mix_at_snr_batch: utterance {u} names noise bank {int(index[u])} of {b_off.size}")
    bo, bl = b_off[index], b_len[index]
    u = first((starts < 0) | (starts + length > bl))
    if u is not None:
        raise ValueError(f"mix_at_snr_batch: utterance {u}: the noise segment [{int(starts[u])}, {int(starts[u] + length[u])}) leaves its bank "
                         f"({int(bl[u])} samples)")
    u = first((bo < 0) | (bo + bl > int(totals[1])))
    if u is not None:
        raise ValueError(f"mix_at_snr_batch: utterance {u}: noise bank {int(index[u])} leaves the noise buffer ({int(totals[1])} elements)")
    if out_layout is None:
        extent = length
        out0 = R.prefix((extent + 63) // 64 * 64)[:-1]
    else:
        out0 = _per_utterance("out0", out_layout[0], U).astype(np.int64)
        extent = _per_utterance("out_extent", out_layout[1], U).astype(np.int64)
        u = first(extent < length)
        if u is not None:
            raise ValueError(f"mix_at_snr_batch: utterance {u}: out_extent {int(extent[u])} is shorter than its {int(length[u])} samples")
        u = first((out0 < 0) | (out0 + extent > int(totals[2])))
        if u is not None:
            raise ValueError(f"mix_at_snr_batch: utterance {u} of the outputs ([{int(out0[u])}, {int(out0[u] + extent[u])})) leaves its buffer "
                             f"({int(totals[2])} elements)")
        order = np.argsort(out0, kind="stable")
        clash = np.flatnonzero(out0[order][:-1] + extent[order][:-1] > out0[order][1:])
        if clash.size:
            a, b = int(order[clash[0]]), int(order[clash[0] + 1])
            raise ValueError(f"mix_at_snr_batch: the output ranges of utterances {a} and {b} overlap")
    return np.concatenate([R.item_prefix(length, MIX_CHUNK), s_off, bo + starts, out0, length, extent]).astype(np.int64)


def condition_grid(n_utts, noise_types, snrs):
    """Every utterance under every noise at every SNR -> (speech_index, noise_index, snr_db), three lists of n_utts x noises x SNRs
    entries, the utterance slowest and the SNR fastest.  noise_types: a count or a list of names (the index is the position)."""
    n_noise = int(noise_types) if isinstance(noise_types, (int, np.integer)) else len(noise_types)
    snrs = [float(s) for s in snrs]
    if n_utts < 1 or n_noise < 1 or not snrs:
        raise ValueError("condition_grid: at least one utterance, one noise and one SNR")
    speech_index, noise_index, snr_db = [], [], []
    for u in range(int(n_utts)):
        for b in range(n_noise):
            for s in snrs:
                speech_index.append(u); noise_index.append(b); snr_db.append(s)
    return speech_index, noise_index, snr_db


def draw_noise_starts(rng, bank_lengths, noise_index, lengths):
    """One segment start per utterance, rng.integers(len(bank) - len(speech)) as packages/dataset/qut_database.py:111 draws it, from a
    numpy.random.Generator.  The reference draws from the global np.random inside a thread pool (create_test_set.py:185-186), so its
    choice of segment depends on the order in which the threads run and is not reproducible: no parity with it is claimed, only the
    same distribution.  ValueError naming the utterance for a bank not longer than its speech."""
    if not isinstance(rng, np.random.Generator):
        raise TypeError("draw_noise_starts: a numpy.random.Generator is required")
    starts = []
    for u, (b, n) in enumerate(zip(noise_index, lengths)):
        room = int(bank_lengths[int(b)]) - int(n)
        if room < 1:
            raise ValueError(f"draw_noise_starts: utterance {u}: noise bank {int(b)} ({int(bank_lengths[int(b)])} samples) is not longer than its "
                             f"{int(n)} samples")
        starts.append(int(rng.integers(room)))
    return starts


def snr_factors(snr_db):
    """np.power(10, -snr_dB / 10) of every utterance, one scalar at a time as create_test_set.py:107 calls it: the reference's bits."""
    return np.array([np.power(10, -float(s) / 10) for s in snr_db], np.float64)


def _entries(x, name):
    """A WaveBatch as it is, anything else as a list of 1-D floating-point arrays / tensors (ragged.as_list in this module's words)."""
    return R.as_list(x, f"mix_at_snr_batch: {name}", R.ENTRY, "nothing given", floating=True)


class MixBatch:
    """What mix_at_snr_batch returns: speech, noise and mixture as WaveBatches over three packed device buffers (one layout: utterance
    u is [offsets[u], offsets[u] + lengths[u]) of each), and stats, the float64 [U, 6] device tensor of p, Ps, Pn, k, norm and the
    achieved SNR in dB per utterance.  plan: the plan_stft_batch layout of the outputs under stft_layout=True, else None."""

    def __init__(self, speech, noise, mixture, stats, snr_db, plan=None):
        self.speech, self.noise, self.mixture, self.stats, self.plan = speech, noise, mixture, stats, plan
        self.snr_db = [float(s) for s in snr_db]

    def __len__(self):
        return len(self.mixture)

    def spec(self, layout=2):
        """The STFT of every mixture (stft.stft_packed on the mixture buffer in place: the end pad is already there) -> SpecBatch,
        bit-identical to stft_batch of the mixtures' host copies."""
        if self.plan is None:
            raise RuntimeError("MixBatch.spec: mix with stft_layout=True to lay the outputs out for the batch STFT")
        p = self.plan
        return H.stft_packed(self.mixture.y, p["frames"], p["x0"], p["padded"], self.mixture.lengths, False, layout)


def mix_packed(speech, noise, tab, factors, normalise_speech=True, out_dtype=torch.float64, n_out=None, outputs=None):
    """dvae_mix_snr_batch on packed device buffers: speech / noise 1-D float32 / float64 CUDA tensors on one device, tab the table of
    mix_tables over them, factors the float64 [U] of snr_factors.  n_out: the element count of each output buffer (default: the end of
    the last output range); outputs: three preallocated 1-D tensors of out_dtype to write into instead.
    -> (out_speech, out_noise, out_mix, stats [U, 6] float64), all on the device."""
    lib = N.load()
    dev = R.check_packed("mix_at_snr_batch", [("speech", speech), ("noise", noise)])
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"mix_at_snr_batch: out_dtype float32 or float64 (got {out_dtype})")
    tab = np.asarray(tab, np.int64)
    U = (tab.size - 1) // 6
    if U < 1 or tab.size != 6 * U + 1:
        raise ValueError(f"mix_at_snr_batch: a table of 6 U + 1 entries is required (got {tab.size})")
    factors = np.asarray(factors, np.float64).reshape(-1)
    if factors.size != U:
        raise ValueError(f"mix_at_snr_batch: {factors.size} SNR factors for {U} utterances")
    n_items = int(tab[U])
    if n_out is None:
        n_out = int(np.max(tab[3 * U + 1:4 * U + 1] + tab[5 * U + 1:6 * U + 1]))
    with torch.cuda.device(dev):
        if outputs is None:
            outputs = [torch.empty(n_out, dtype=out_dtype, device=dev) for _ in range(3)]
        for o in outputs:
            if not (torch.is_tensor(o) and o.is_cuda and o.device == dev and o.dim() == 1 and o.dtype == out_dtype and o.is_contiguous()
                    and o.numel() == n_out):
                raise TypeError(f"mix_at_snr_batch: every output must be a contiguous 1-D {out_dtype} tensor of {n_out} elements on {dev}")
        stats = torch.empty((U, 6), dtype=torch.float64, device=dev)
        ws = torch.empty(lib.dvae_mix_snr_workspace_bytes(n_items, U), dtype=torch.uint8, device=dev)
        tab_dev, fac_dev = R.upload(tab, dev), R.upload(factors, dev)
        f64 = R.f64_flag
        N.check(lib.dvae_mix_snr_batch(N.ptr(speech), speech.numel(), f64(speech), N.ptr(noise), noise.numel(), f64(noise), U, N.ptr(tab_dev),
                                       n_items, N.ptr(fac_dev), 1 if normalise_speech else 0, N.ptr(outputs[0]), N.ptr(outputs[1]),
                                       N.ptr(outputs[2]), n_out, 1 if out_dtype == torch.float64 else 0, N.ptr(stats), N.ptr(ws), N.stream()),
                "dvae_mix_snr_batch")
    return outputs[0], outputs[1], outputs[2], stats


def mix_at_snr_batch(speech, noise_banks, noise_index, starts, snr_db, normalise_speech=True, out_dtype=torch.float64, stft_layout=False):
    """process_save_utt (scripts/create_test_set.py:89-125) of every utterance in five launches.

    speech: a WaveBatch (its ranges may repeat) or a list of 1-D numpy arrays / tensors, one entry per mixture (float32 or float64;
    host lists are packed into one pinned buffer and uploaded once, an array that appears several times only once).  noise_banks: a
    list of long 1-D recordings, packed once (a single device tensor is adopted without a copy), or a WaveBatch of them.
    noise_index[u] / starts[u]: the bank of utterance u and the first sample of its segment there (draw_noise_starts draws them);
    snr_db[u]: its target SNR.  normalise_speech=False skips the division of the speech by its peak.  out_dtype: float64, or float32
    (one more rounding of the double result).  stft_layout=True lays the three outputs out as plan_stft_batch lays out padded signals
    (center=False, the end pad of hop zeros written by the kernel), so that MixBatch.spec() transforms the mixtures in place.
    -> MixBatch.  Nothing is synchronised: the call enqueues on the current stream."""
    speech = _entries(speech, "speech")
    if not isinstance(noise_banks, H.WaveBatch):          # a WaveBatch of banks is taken as it is: mix_packed checks its buffer
        noise_banks = _entries(noise_banks, "noise_banks")
    s_view, b_view = R.view(speech, dedupe=True), R.view(noise_banks, dedupe=True)
    U = len(s_view[0])
    # every refusal comes before anything is uploaded or the library is loaded
    snr_db = _per_utterance("snr_db", np.asarray(snr_db, np.float64), U)
    plan = H.plan_stft_batch(s_view[1], center=False, pad_at_end=True) if stft_layout else None
    layout = None if plan is None else (plan["x0"], plan["padded"])
    n_out = None if plan is None else int(plan["padded"].sum())
    tab = mix_tables(s_view[:2], (b_view[0], b_view[1], noise_index), starts, None, (s_view[2], b_view[2], n_out), layout)
    factors = snr_factors(snr_db)
    dev = R.find_device(speech, noise_banks)
    with torch.cuda.device(dev):
        s_buf = R.pack(speech, "mix_at_snr_batch: speech", dev, R.ENTRY, dedupe=True)
        b_buf = R.pack(noise_banks, "mix_at_snr_batch: noise_banks", dev, R.ENTRY, dedupe=True)
    out_s, out_n, out_x, stats = mix_packed(s_buf, b_buf, tab, factors, normalise_speech, out_dtype, n_out)
    out0, lengths = tab[3 * U + 1:4 * U + 1], tab[4 * U + 1:5 * U + 1]
    return MixBatch(*(H.WaveBatch(o, out0, lengths) for o in (out_s, out_n, out_x)), stats, snr_db, plan)
