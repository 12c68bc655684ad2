"""Drop-in surface of the reference's packages/metrics.py scale-invariant scores: si_sdr_components, energy_ratios, si_sdr_leroux
(same names, same argument order).  Host arrays are scored with numpy on the host (the reference's CPU mode: the data never was on
a device); CUDA tensors go to the HIP library as a batch of one (disentangled-vae_amd/metrics.py) or raise, never to a host copy.
mean_confidence_interval / compute_stats (printing, scipy) are not part of this surface.
"""
import numpy as np
import torch

from . import _native


def _where(*arrays):
    """'cuda' if every argument is a CUDA tensor, 'host' if none is; a mixture is refused."""
    on = [torch.is_tensor(a) and a.is_cuda for a in arrays]
    if all(on):
        return "cuda"
    if any(on):
        raise TypeError("metrics: host arrays and CUDA tensors mixed in one call")
    return "host"


def _host(a):
    return a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)


def _scale(s_hat, ref):
    """The projection coefficient of s_hat on ref: <s_hat, ref> / |ref|^2."""
    return np.dot(s_hat, ref) / np.linalg.norm(ref) ** 2


def _energy(x):
    return np.linalg.norm(x) ** 2


def si_sdr_components(s_hat, s, n):
    """s_hat = s_target + e_noise + e_art with s_target = alpha_s s and e_noise = alpha_n n, each alpha the projection of s_hat on
    that signal alone.  -> (s_target, e_noise, e_art).  Host arrays only: the device scorer never forms the components as arrays
    (energy_ratios and disentangled-vae_amd/metrics.py: energy_ratios_batch return their energies)."""
    if _where(s_hat, s, n) == "cuda":
        raise TypeError("si_sdr_components: the component waveforms exist on the host path only; on CUDA tensors use energy_ratios "
                        "(or energy_ratios_batch(..., return_sums=True) for the component energies)")
    s_hat, s, n = _host(s_hat), _host(s), _host(n)
    s_target = _scale(s_hat, s) * s
    e_noise = _scale(s_hat, n) * n
    e_art = s_hat - s_target - e_noise
    return s_target, e_noise, e_art


def energy_ratios(s_hat, s, n):
    """(SI-SDR, SI-SIR, SI-SAR) in dB: the energy of s_target over that of e_noise + e_art, of e_noise, of e_art.  (SI-SIR is the
    SI-SNR: the noise is the only interfering source.)  CUDA tensors -> three 0-d float64 CUDA tensors from the HIP scorer."""
    if _where(s_hat, s, n) == "cuda":
        return tuple(_native.metrics_dev().energy_ratios_batch([s_hat], [s], [n])[0].unbind())
    s_target, e_noise, e_art = si_sdr_components(s_hat, s, n)
    target = _energy(s_target)
    si_sdr = 10 * np.log10(target / _energy(e_noise + e_art))
    si_sir = 10 * np.log10(target / _energy(e_noise))
    si_sar = 10 * np.log10(target / _energy(e_art))
    return si_sdr, si_sir, si_sar


def si_sdr_leroux(s_hat, s):
    """SI-SDR in dB without a noise reference: the energy of s_target = alpha_s s over that of s_target - s_hat.  CUDA tensors -> a
    0-d float64 CUDA tensor from the HIP scorer."""
    if _where(s_hat, s) == "cuda":
        return _native.metrics_dev().si_sdr_batch([s_hat], [s])[0]
    s_hat, s = _host(s_hat), _host(s)
    s_target = _scale(s_hat, s) * s
    return 10 * np.log10(_energy(s_target) / _energy(s_target - s_hat))
