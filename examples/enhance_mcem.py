"""Speech enhancement of a batch of utterances on the MI355X-native path: the per-utterance flow of the reference's
scripts/evaluate_ntcd_M2.py:139-230 (STFT -> MCEM with a VAE speech prior and an NMF noise model -> Wiener
filtering -> ISTFT), for many utterances at once (disentangled-vae_amd/mcem.py: McemBatch), with nothing leaving the
device between the batch STFT and the waveforms.

    python examples/enhance_mcem.py --wav a.wav b.wav --checkpoint models/M2_epoch_118_vloss_407.90.pt --out enhanced/
    python examples/enhance_mcem.py --synthetic 8                       # no data at hand: modulated-noise "speech" + noise
    python examples/enhance_mcem.py --synthetic 8 --score               # and SI-SDR and ESTOI of mixture and estimate, scored on the device
    python examples/enhance_mcem.py --synthetic 8 --snr -5 0 5 --score  # every utterance mixed on the device at each SNR (create_test_set.py's
                                                                        # mixing: disentangled-vae_amd/mix.py); --score adds SI-SIR and SI-SAR

    python examples/enhance_mcem.py --synthetic 8 --labels classifier --score   # the M2_info flow: labels from the model's own classifier

    python examples/enhance_mcem.py --synthetic 3 --z-dim 32 --h-dim 256 64 --fused-start --labels classifier --score
                                                                        # a model of another size: the generic kernels for classifier,
                                                                        # encoder and chain (pack_classifier / pack_encoder pick them)

--labels vad (the default): the labels y fed to the M2 decoder are the time-domain VAD of the mixture
(packages/processing/target.py); the reference's evaluate_ntcd_M2.py takes them from a video classifier or from the clean signal
(oracle), neither of which ships with it.  --labels classifier: the flow of scripts/evaluate_ntcd_M2_info_vad.py:175-219 -- a
DeepGenerativeModel_v5 (M2_info) whose classifier labels every frame of the mixtures' SpecBatch in one launch
(disentangled-vae_amd/classify.py: classify_batch), the hard labels going to the M2v3 variant of MCEM device to device; --score
then adds the F1 of those labels against the clean speech's VAD (f1_batch).  Writes <name>_s_est.wav and <name>_n_est.wav like the reference (evaluate_ntcd_M2.py:232-245).
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from packages.models.models import DeepGenerativeModel, DeepGenerativeModel_v5
from packages.processing.target import clean_speech_VAD

McemBatch = importlib.import_module("disentangled-vae_amd.mcem").McemBatch
stft_batch = importlib.import_module("disentangled-vae_amd.stft").stft_batch
si_sdr_batch = importlib.import_module("disentangled-vae_amd.metrics").si_sdr_batch
estoi_batch = importlib.import_module("disentangled-vae_amd.metrics").estoi_batch
mix_at_snr_batch = importlib.import_module("disentangled-vae_amd.mix").mix_at_snr_batch
classify = importlib.import_module("disentangled-vae_amd.classify")
encode = importlib.import_module("disentangled-vae_amd.encode")
utterances_to_frames = importlib.import_module("disentangled-vae_amd.target").utterances_to_frames
STFT = dict(fs=16000, wlen_sec=64e-3, win="hann", hop_percent=0.25, center=False)      # evaluate_ntcd_M2.py:37-45


def synthetic_mixture(seconds, seed):
    """-> (mixture, speech, noise), mixture = speech + noise."""
    rng = np.random.default_rng(seed)
    n = int(16000 * seconds)
    env = np.repeat((rng.random(n // 800 + 1) > 0.5).astype(np.float64), 800)[:n]      # 50 ms on/off "speech"
    s = env * rng.standard_normal(n) * np.sin(2 * np.pi * 220 * np.arange(n) / 16000 + rng.random())
    noise = 0.2 * rng.standard_normal(n)
    return s + noise, s, noise


def synthetic_noise_banks(seconds, seed, count=2):
    """`count` long noise recordings: white noise through one-pole low-pass filters of different corners."""
    rng = np.random.default_rng(seed)
    banks = []
    for b in range(count):
        w = rng.standard_normal(int(16000 * seconds))
        a = 0.5 + 0.4 * b / max(count - 1, 1)
        for i in range(1, 4):
            w[i:] += a ** i * w[:-i]                      # a short FIR stand-in for the filter: no sample-by-sample loop
        banks.append(0.1 * w)
    return banks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", nargs="*", default=[])
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic 3-4 s mixtures instead of --wav")
    ap.add_argument("--checkpoint", default=None, help="M2 (y_dim 1) state_dict, or M2_info with --labels classifier; random weights when absent")
    ap.add_argument("--labels", choices=["vad", "classifier"], default="vad", help="where the decoder's labels come from: the mixture's "
                    "time-domain VAD, or the classifier of an M2_info model on the device")
    ap.add_argument("--niter", type=int, default=100)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--out", default="enhanced")
    ap.add_argument("--fused-start", action="store_true", help="McemBatch.init_parameters(fused_start=True): the start of the EM loop in a fixed "
                    "number of launches (one encoder launch for Z, one draw each for W and H); another draw order than the default")
    ap.add_argument("--std-norm", default=None, metavar="NORM_PT", help="with --fused-start: the encoder was trained on standardised input "
                    "(examples/train_fused.py --std-norm); the norm.pt written there (X_train_mean / X_train_std) goes into the encoder pack")
    ap.add_argument("--score", action="store_true", help="with --synthetic (whose speech is known): SI-SDR and ESTOI of mixture and estimate per utterance")
    ap.add_argument("--snr", type=float, nargs="+", default=None, help="with --synthetic: mix every utterance with synthetic noise at each of "
                    "these SNRs (dB) on the device instead of adding a fixed 0.2 * randn on the host")
    ap.add_argument("--z-dim", type=int, default=16, help="latent size of the model, random-weight or --checkpoint (any 1..128: sizes other than the "
                    "reference's 16 / 128 / 128 run the generic fp32 kernels -- chain, encoder of --fused-start, classifier of --labels classifier)")
    ap.add_argument("--h-dim", type=int, nargs=2, default=[128, 128], metavar=("H1", "H2"), help="hidden widths of the model (1..512 each); examples/train_fused.py "
                    "--z-dim / --h-dim trains and saves such a model")
    ap.add_argument("--trim", type=int, default=800, help="samples cut at both ends before scoring (run_metrics.py:117-121: 0.05 s)")
    a = ap.parse_args()
    if a.score and (a.wav or not a.synthetic):
        ap.error("--score needs the clean speech, which only --synthetic mixtures come with")
    if a.snr is not None and (a.wav or not a.synthetic):
        ap.error("--snr mixes the --synthetic utterances")
    if (a.z_dim, list(a.h_dim)) != (16, [128, 128]) and a.precision != "fp32":
        ap.error("--z-dim / --h-dim: sizes other than 16 / 128 128 run the generic kernels, which are fp32 (mcem.chain_kind, "
                 "encode.encoder_kind, classify.classifier_kind)")
    names, waves, clean = [], [], []
    for p in a.wav:
        fs, w = wavfile.read(p)
        assert fs == 16000, f"{p}: 16 kHz expected"
        waves.append(w.astype(np.float64) / (32768.0 if w.dtype == np.int16 else 1.0)); names.append(os.path.splitext(os.path.basename(p))[0])
    for i in range(a.synthetic if not a.wav else 0):
        mix, speech, _ = synthetic_mixture(3.0 + 0.25 * (i % 5), i)
        waves.append(mix); clean.append(speech); names.append(f"synthetic_{i:02d}")
    if not waves:
        ap.error("give --wav files or --synthetic N")
    torch.manual_seed(0)
    sizes = [513, 1, a.z_dim, list(a.h_dim)]
    vae = DeepGenerativeModel_v5(sizes) if a.labels == "classifier" else DeepGenerativeModel(sizes, None)
    if a.checkpoint:
        vae.load_state_dict(torch.load(a.checkpoint, map_location="cpu", weights_only=True))
    vae = vae.cuda().eval()
    for p in vae.parameters():
        p.requires_grad = False

    t0 = time.perf_counter()
    mix = None
    if a.snr is not None:
        # every utterance at every SNR in one call, the noise segments drawn from two banks: speech, noise (at the mixture's scale) and
        # mixture stay on the device, the mixtures laid out for the batch STFT with their end pad written by the kernel
        mixer = importlib.import_module("disentangled-vae_amd.mix")
        banks = synthetic_noise_banks(8.0, 1000)
        speech = [clean[u] for u in range(len(clean)) for _ in a.snr]
        names = [f"{names[u]}_snr{snr:+g}" for u in range(len(clean)) for snr in a.snr]
        noise_index = [u % len(banks) for u in range(len(clean)) for _ in a.snr]
        snr_db = [snr for _ in clean for snr in a.snr]
        starts = mixer.draw_noise_starts(np.random.default_rng(0), [len(b) for b in banks], noise_index, [len(s) for s in speech])
        mix = mix_at_snr_batch(speech, banks, noise_index, starts, snr_db, stft_layout=True)
        X = mix.spec()
        waves = mix.mixture.numpy()                       # one download: the VAD labels below are made on the host
        clean = mix.speech
    else:
        # every mixture's STFT in one launch, kept on the device: (513, N_u) complex64 per utterance, frame-major and packed
        X = stft_batch(waves, pad_mode="reflect", pad_at_end=True, **STFT)
    if a.labels == "classifier":
        # y_hat_soft = model.classifier(|X|^2), y_hat_hard = y_hat_soft > 0.5 for every frame of the batch in one launch; the LabelBatch
        # stays on the device and MCEM_M2v3 (labels in the decoder only) takes its hard labels from there
        # (pack_classifier: the resident kernel at 513-128-128, the generic one at every other covered size)
        Y = classify.classify_batch(classify.pack_classifier(vae.enc_dec_clf.classifier), X)
        mb = McemBatch(vae.enc_dec_clf, niter=a.niter, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75, var_RW=0.01,
                       nmf_rank=10, precision=a.precision, label_in_encoder=False, label_in_decoder=True)
    else:
        Y = [clean_speech_VAD(w, fs=16000, wlen_sec=64e-3, hop_percent=0.25, center=False, pad_mode="reflect", pad_at_end=True,
                              vad_threshold=1.70) for w in waves]                                              # (1, N_u)
        mb = McemBatch(vae, niter=a.niter, nsamples_E_step=10, burnin_E_step=30, nsamples_WF=25, burnin_WF=75, var_RW=0.01,
                       nmf_rank=10, precision=a.precision)                                                      # evaluate_ntcd_M2.py:92-99
    # the fused start's encoder by its kind too: labels reach the encoder of M2 (y_dim 1), not that of M2_info's M2v3 variant
    norm = None
    if a.std_norm:
        if not a.fused_start:
            ap.error("--std-norm applies to --fused-start (the encoder pack carries the statistics)")
        st = torch.load(a.std_norm, map_location="cpu")
        norm = (st["X_train_mean"], st["X_train_std"])
    enc_pack = encode.pack_encoder(mb.vae.encoder, 1 if mb.label_in_encoder else 0, norm=norm) if a.fused_start else None
    mb.init_parameters(X, Y, fused_start=a.fused_start, encoder_pack=enc_pack)
    cost = mb.run()
    # Wiener filtering and ISTFT of both estimates in one launch: istft(S_hat, max_len=len(w)) / istft(N_hat, ...) per utterance
    s_hat, n_hat = mb.enhance(max_len=[len(w) for w in waves])
    os.makedirs(a.out, exist_ok=True)
    for name, s_u, n_u in zip(names, s_hat.numpy(), n_hat.numpy()):
        wavfile.write(os.path.join(a.out, name + "_s_est.wav"), 16000, s_u.astype(np.float32))
        wavfile.write(os.path.join(a.out, name + "_n_est.wav"), 16000, n_u.astype(np.float32))
    dt = time.perf_counter() - t0
    frames = sum(X.counts)
    print(f"{len(waves)} utterances, {frames} frames, {a.niter} EM iterations: {dt:.2f} s wall ({len(waves) / dt:.1f} utterances/s); "
          f"cost {cost[0].mean():.3f} -> {cost[-1].mean():.3f}")
    if a.score:
        # scored on the device (si_sdr_leroux of every utterance in three launches); only the two [U] results come back
        sdr_est = mb.score(clean, max_len=[len(w) for w in waves], trim=a.trim).cpu().numpy()
        sdr_mix = si_sdr_batch(waves if mix is None else mix.mixture, clean, trim=a.trim).cpu().numpy()
        # and the intelligibility (ESTOI as include/dvae.h writes it out, six launches): the clean speech first, as pystoi takes it
        ei_est = mb.estoi(clean, max_len=[len(w) for w in waves], trim=a.trim).cpu().numpy()
        ei_mix = estoi_batch(clean, waves if mix is None else mix.mixture, STFT["fs"], trim=a.trim).cpu().numpy()
        print(f"{'utterance':<16}{'SI-SDR mixture':>16}{'SI-SDR estimate':>17}   (dB){'ESTOI mixture':>16}{'ESTOI estimate':>16}")
        for name, m, e, im, ie in zip(names, sdr_mix, sdr_est, ei_mix, ei_est):
            print(f"{name:<16}{m:>16.2f}{e:>17.2f}{'':>7}{im:>16.3f}{ie:>16.3f}")
        print(f"{'mean':<16}{sdr_mix.mean():>16.2f}{sdr_est.mean():>17.2f}{'':>7}{ei_mix.mean():>16.3f}{ei_est.mean():>16.3f}")
        if a.labels == "classifier":
            # the labels' score against the clean speech's VAD (run_metrics_classif.py:136), counted on the device; the truth's frames
            # are those of the mixtures' STFT (the same lengths and the same end pad)
            truth = utterances_to_frames(clean.numpy() if mix is not None else clean, "vad_labels", device="cuda")
            f1 = classify.f1_batch(Y, truth).cpu().numpy()
            print(f"{'utterance':<24}{'accuracy':>10}{'precision':>11}{'recall':>10}{'F1':>10}")
            for name, r in zip(names, f1):
                print(f"{name:<24}{r[0]:>10.3f}{r[1]:>11.3f}{r[2]:>10.3f}{r[3]:>10.3f}")
        if mix is not None:
            # the mixer's noise is at the mixture's scale, which is what SI-SIR and SI-SAR need (energy_ratios, packages/metrics.py:39-60)
            ratios = mb.score(mix.speech, mix.noise, max_len=[len(w) for w in waves], trim=a.trim).cpu().numpy()
            achieved = mix.stats[:, 5].cpu().numpy()
            print(f"{'utterance':<24}{'SNR (dB)':>10}{'SI-SDR':>10}{'SI-SIR':>10}{'SI-SAR':>10}")
            for name, snr, r in zip(names, achieved, ratios):
                print(f"{name:<24}{snr:>10.2f}{r[0]:>10.2f}{r[1]:>10.2f}{r[2]:>10.2f}")


if __name__ == "__main__":
    main()
