"""The VAE encoder for a ragged batch on the device: the latent start of the MCEM loop and the encoding half of the reference's
reconstruction / disentanglement analysis.

encode_batch runs `vae.encoder` (packages/models/models.py: Encoder([513 + y_dim, [128, 128], 16]): tanh, tanh, the mu and log_var
heads) over every frame of a SpecBatch in ONE launch (include/dvae.h: dvae_encode_batch) -- the reference's `_, Z, _ =
vae.encoder(torch.t(X2))` (packages/models/mcem.py:200, 364) and the `model.encoder(...)` calls of scripts/reconstruct_ntcd_M2.py:231-358
and reconstruct_M2_info.py, |X|^2 formed in the kernel with the bits of McemBatch.X2, the labels of M2 read as rows beside the frames
(no torch.cat).  reconstruct_batch decodes the latents with DecoderPack.decode under any label, which is what those scripts plot.
encode_rows is the thin call on device buffers; with the column output it writes mu straight into McemBatch's Z [16, ntot]
(McemBatch.init_parameters(fused_start=True)).  No CPU arithmetic exists here: without the library or a GPU the batch ops raise;
encoder_supported, LatentBatch and the table checks on host tensors need neither.
"""
import numpy as np
import torch
from torch import nn

from . import native as N
from . import ragged as R
from . import stft as STFT
from . import target as TGT
from .classify import LabelBatch, frame_table, _rows

F_BINS, H_DIM, Z_DIM = 513, 128, 16
Y_DIMS = (0, 1, F_BINS)
Z_MAX, H_MAX = 128, 512                         # limits of the generic kernel (csrc/mlp_generic.hip), those of dvae_mcem_plan_dims


def _shape(enc):
    """What encoder_supported looks at, as a string for the refusal."""
    hidden, sample = getattr(enc, "hidden", None), getattr(enc, "sample", None)
    if hidden is None or sample is None:
        return f"{type(enc).__name__} (no hidden / sample)"
    parts = [f"{l.in_features}->{l.out_features}" if isinstance(l, nn.Linear) else type(l).__name__ for l in hidden]
    for head in (getattr(sample, "mu", None), getattr(sample, "log_var", None)):
        parts.append(f"{head.in_features}->{head.out_features}" if isinstance(head, nn.Linear) else type(head).__name__)
    return f"{type(enc).__name__} [{', '.join(parts)}]"


def encoder_supported(encoder, y_dim):
    """The kernel covers the encoder the reference's scripts build: Encoder([513 + y_dim, [128, 128], 16]) with a GaussianSample
    layer, y_dim 0 (M1, and the x-only encoders of DeepGenerativeModel_v3 / _v5), 1 or 513 (M2)."""
    from packages.models.models import Encoder, GaussianSample
    if not isinstance(encoder, Encoder) or y_dim not in Y_DIMS or type(encoder.sample) is not GaussianSample:
        return False
    hs = list(encoder.hidden)
    heads = [encoder.sample.mu, encoder.sample.log_var]
    return (len(hs) == 2 and all(isinstance(l, nn.Linear) and l.bias is not None for l in hs + heads)
            and hs[0].in_features == F_BINS + y_dim and hs[0].out_features == H_DIM and hs[1].in_features == H_DIM and hs[1].out_features == H_DIM
            and all(l.in_features == H_DIM and l.out_features == Z_DIM for l in heads))


def _generic_dims(encoder, y_dim):
    """(h1, h2, z_dim) where the generic kernel covers the encoder, else None: an Encoder with a GaussianSample layer and two hidden
    Linear layers with biases, [513 + y_dim] -> h1 -> h2 -> {mu z, log_var z} within the limits."""
    from packages.models.models import Encoder, GaussianSample
    if not isinstance(encoder, Encoder) or type(getattr(encoder, "sample", None)) is not GaussianSample:
        return None
    y_dim = int(y_dim)
    hs = list(encoder.hidden)
    heads = [encoder.sample.mu, encoder.sample.log_var]
    if len(hs) != 2 or not all(isinstance(l, nn.Linear) and l.bias is not None for l in hs + heads):
        return None
    h1, h2, z = hs[0].out_features, hs[1].out_features, heads[0].out_features
    if hs[0].in_features != F_BINS + y_dim or hs[1].in_features != h1 or any(l.in_features != h2 or l.out_features != z for l in heads):
        return None
    if not (0 <= y_dim <= F_BINS and 1 <= h1 <= H_MAX and 1 <= h2 <= H_MAX and 1 <= z <= Z_MAX):
        return None
    return h1, h2, z


def encoder_kind(encoder, y_dim):
    """Which kernel serves `encoder` fed [x | y_dim label columns]: "resident" (encode.hip: the reference's geometry,
    encoder_supported), "generic" (csrc/mlp_generic.hip: two hidden layers, hidden widths 1..512, z_dim 1..128, y_dim 0..513, 513
    bins, fp32) or None.  Reads layer shapes only: works on CPU modules."""
    if _generic_dims(encoder, y_dim) is None:
        return None
    return "resident" if encoder_supported(encoder, y_dim) else "generic"


class EncoderPack:
    """The eight state_dict tensors of an Encoder in one contiguous float32 device buffer, the layout of dvae_encode_batch:
    W1 [128][513 + y_dim] | b1 | W2 [128][128] | b2 | Wmu [16][128] | bmu | Wlv [16][128] | blv.  repack(encoder) after training.
    generic=True: the fragment-order copy of dvae_encode_generic_pack for the generic kernel, which covers every geometry
    encoder_kind names (the reference's too); z_dim, h1, h2, y_dim: the geometry.
    norm=(mean, std) (513 floats each, as GenericTrainer's std_norm; norm_eps as there): the pack of an encoder trained on
    standardised input -- always the generic one --, whose x block is (x - mean) / (std + norm_eps) formed in the kernel after the
    power, torch's float32 bits (dvae_encode_generic_batch_norm); labels are not normalised."""

    def __init__(self, encoder, y_dim, generic=False, norm=None, norm_eps=1e-8):
        self.generic = bool(generic) or norm is not None
        self.norm = None
        if norm is not None:
            from .trainer_generic import check_std_norm
            self._norm_host = check_std_norm(norm, norm_eps, "EncoderPack: norm")[:2]
        if self.generic:
            dims = _generic_dims(encoder, y_dim)
            if dims is None:
                raise TypeError(f"encode_batch: the generic kernel covers Encoder [513+y->h1, h1->h2, h2->z, h2->z] with y_dim 0..{F_BINS}, "
                                f"h1 / h2 1..{H_MAX}, z 1..{Z_MAX}, got {_shape(encoder)} with y_dim {y_dim}")
            self.h1, self.h2, self.z_dim = dims
        else:
            if not encoder_supported(encoder, y_dim):
                raise TypeError(f"encode_batch: the kernel covers Encoder [513+y->128, 128->128, 128->16, 128->16] with y_dim 0, 1 or 513, "
                                f"got {_shape(encoder)} with y_dim {y_dim}")
            self.h1, self.h2, self.z_dim = H_DIM, H_DIM, Z_DIM
        self.y_dim = int(y_dim)
        self.weights = None
        self.repack(encoder)

    def repack(self, encoder):
        ts = [p.detach() for l in (*encoder.hidden, encoder.sample.mu, encoder.sample.log_var) for p in (l.weight, l.bias)]
        if not all(t.is_cuda for t in ts):
            raise RuntimeError("encode_batch: the encoder's parameters must be CUDA tensors (no CPU fallback)")
        if any(t.dtype != torch.float32 for t in ts):
            raise TypeError("encode_batch: the HIP path computes in float32")
        if self.generic:
            if _generic_dims(encoder, self.y_dim) != (self.h1, self.h2, self.z_dim):
                raise TypeError(f"encode_batch: repack: {_shape(encoder)} is not the geometry this pack was made for")
            lib = N.load()
            want = lib.dvae_encode_generic_weights_floats(self.y_dim, self.h1, self.h2, self.z_dim)
            dev = ts[0].device
            if self.weights is None or self.weights.device != dev:
                self.weights = torch.empty(want, dtype=torch.float32, device=dev)
            ts = [t.contiguous() for t in ts]
            with torch.cuda.device(dev):
                N.check(lib.dvae_encode_generic_pack(self.y_dim, self.h1, self.h2, self.z_dim, N.ptr(ts[0]), ts[0].stride(0), N.ptr(ts[1]),
                                                     N.ptr(ts[2]), ts[2].stride(0), N.ptr(ts[3]), N.ptr(ts[4]), ts[4].stride(0), N.ptr(ts[5]),
                                                     N.ptr(ts[6]), ts[6].stride(0), N.ptr(ts[7]), N.ptr(self.weights), N.stream()),
                        "dvae_encode_generic_pack")
            self._keep = ts                  # the pack kernels read them on the stream
            if getattr(self, "_norm_host", None) is not None and (self.norm is None or self.norm[0].device != dev):
                self.norm = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in self._norm_host)      # (mean, div)
            return
        flat = torch.cat([t.reshape(-1) for t in ts])
        want = N.load().dvae_encode_weights_floats(self.y_dim)
        if flat.numel() != want:
            raise RuntimeError(f"encode_batch: packed {flat.numel()} floats, the kernel reads {want}")
        if self.weights is None or self.weights.device != flat.device:
            self.weights = flat
        else:
            self.weights.copy_(flat)


def pack_encoder(encoder, y_dim, norm=None, norm_eps=1e-8):
    """The pack of `encoder` by encoder_kind: the resident pack wherever it applies, the generic one for every other covered
    geometry and whenever norm=(mean, std) is given; TypeError naming the shape and the limits for an encoder no kernel covers."""
    kw = {} if norm is None else dict(norm=norm, norm_eps=norm_eps)
    return EncoderPack(encoder, y_dim, generic=encoder_kind(encoder, y_dim) != "resident", **kw)


class LatentBatch:
    """The latents of a ragged batch on the device, frame-major: mu, log_var float32 [N, z_dim], z [N, z_dim] or None (no eps
    given), utterance u at rows frame_off[u] : frame_off[u + 1]; counts: T_u.  view(u, which): the (z_dim, T_u) view of "mu",
    "log_var" or "z", the orientation the reference's scripts hold latents in."""

    def __init__(self, mu, log_var, z, counts, frame_off=None):
        self.mu, self.log_var, self.z = mu, log_var, z
        self.counts = [int(c) for c in counts]
        self.frame_off = R.prefix(self.counts) if frame_off is None else np.asarray(frame_off, np.int64)

    def __len__(self):
        return len(self.counts)

    def _which(self, which):
        if which not in ("mu", "log_var", "z"):
            raise ValueError(f"LatentBatch: use 'mu', 'log_var' or 'z', got {which!r}")
        t = getattr(self, which)
        if t is None:
            raise ValueError(f"LatentBatch: no {which} (encode_batch without eps forms no z)")
        return t

    def view(self, u, which="mu"):
        return self._which(which)[int(self.frame_off[u]):int(self.frame_off[u + 1])].T

    def numpy(self, which="mu"):
        """Every utterance as a host array (16, T_u) (views of one host copy)."""
        h = self._which(which).cpu().numpy()
        return [h[a:b].T for a, b in zip(self.frame_off[:-1], self.frame_off[1:])]


def column_table(op, frame_off, cols, ntot):
    """The int64 first columns [U] of utterances written side by side into [., ntot] columns: ValueError naming the utterance for
    columns that go back or leave ntot (what dvae_encode_batch checks again)."""
    off = np.asarray(frame_off, np.int64).reshape(-1)
    cols = np.asarray(cols, np.int64).reshape(-1)
    if cols.size != off.size - 1:
        raise ValueError(f"{op}: {cols.size} first columns for {off.size - 1} utterances")
    end = 0
    for u, c0 in enumerate(cols):
        c = int(off[u + 1] - off[u])
        if c0 < end:
            raise ValueError(f"{op}: utterance {u} starts at column {int(c0)}, {end} are taken")
        if c0 + c > int(ntot):
            raise ValueError(f"{op}: utterance {u} (columns [{int(c0)}, {int(c0) + c})) leaves the {int(ntot)} columns given")
        end = int(c0) + c
    return cols


def _out_ok(op, name, o, n_rows, dev, z_dim=Z_DIM):
    if o is not None and not (torch.is_tensor(o) and o.is_cuda and o.device == dev and o.dtype == torch.float32 and o.is_contiguous()
                              and tuple(o.shape) == (n_rows, z_dim)):
        raise ValueError(f"{op}: {name} must be contiguous float32 CUDA rows [{n_rows}, {z_dim}] beside the frames")


def encode_rows(pack, src, frame_off, y=None, eps=None, mu=None, log_var=None, z=None, Z=None, cols=None, tables_dev=None):
    """dvae_encode_batch on device buffers: src complex64 [N, 513] frames or float32 [N, >= 513 by stride] power rows, frame_off the
    host prefix [U + 1], y float32 label rows [N, y_dim by stride] (exactly when the pack has y_dim > 0), eps / mu / log_var / z
    float32 [N, 16], written in place for the rows inside the table and nowhere else.  Z float32 [16, ntot] with cols, the first
    column of every utterance: mu transposed into McemBatch's layout, the other columns untouched (tables_dev: the device table
    [frame_off | cols] if the caller has it already, e.g. from dvae_mcem_spec_init).  With a generic pack the same through
    dvae_encode_generic_batch, 16 being the pack's z_dim."""
    op = "encode_batch"
    lib = N.load()
    is_complex = src.dtype == torch.complex64
    ld = F_BINS if is_complex else N.ld(src)
    n = src.shape[0]
    off = np.ascontiguousarray(frame_off, np.int64)
    if (pack.y_dim > 0) != (y is not None):
        raise ValueError(f"{op}: labels are needed exactly when the encoder takes them (y_dim {pack.y_dim})")
    if y is not None and not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape == (n, pack.y_dim) and y.stride(1) == 1
                              and (n == 1 or y.stride(0) >= pack.y_dim)):
        raise ValueError(f"{op}: labels must be float32 CUDA rows [{n}, {pack.y_dim}]")
    for name, o in (("eps", eps), ("mu", mu), ("log_var", log_var), ("z", z)):
        _out_ok(op, name, o, n, src.device, pack.z_dim)
    if z is not None and eps is None:
        raise ValueError(f"{op}: z needs eps")
    ntot, col = 0, None
    if Z is not None:
        if not (Z.is_cuda and Z.dtype == torch.float32 and Z.is_contiguous() and Z.dim() == 2 and Z.shape[0] == pack.z_dim):
            raise ValueError(f"{op}: Z must be a contiguous float32 CUDA tensor [{pack.z_dim}, ntot]")
        ntot = Z.shape[1]
        col = np.ascontiguousarray(column_table(op, off, cols, ntot))
        if tables_dev is None:
            tables_dev = R.upload(np.concatenate([off, col]), src.device)
    with torch.cuda.device(src.device):
        if pack.generic and pack.norm is not None:
            N.check(lib.dvae_encode_generic_batch_norm(N.ptr(src), int(is_complex), ld, N.ptr(y), N.ld(y) if y is not None else 0, n, off.size - 1,
                                                       off.ctypes.data, N.ptr(pack.weights), pack.y_dim, pack.h1, pack.h2, pack.z_dim, N.ptr(eps),
                                                       N.ptr(mu), N.ptr(log_var), N.ptr(z), N.ptr(Z), ntot,
                                                       col.ctypes.data if col is not None else None,
                                                       N.ptr(tables_dev) if Z is not None else None, N.ptr(pack.norm[0]), N.ptr(pack.norm[1]),
                                                       N.stream()), "dvae_encode_generic_batch_norm")
            return
        if pack.generic:
            N.check(lib.dvae_encode_generic_batch(N.ptr(src), int(is_complex), ld, N.ptr(y), N.ld(y) if y is not None else 0, n, off.size - 1,
                                                  off.ctypes.data, N.ptr(pack.weights), pack.y_dim, pack.h1, pack.h2, pack.z_dim, N.ptr(eps), N.ptr(mu),
                                                  N.ptr(log_var), N.ptr(z), N.ptr(Z), ntot, col.ctypes.data if col is not None else None,
                                                  N.ptr(tables_dev) if Z is not None else None, N.stream()), "dvae_encode_generic_batch")
            return
        N.check(lib.dvae_encode_batch(N.ptr(src), int(is_complex), ld, N.ptr(y), N.ld(y) if y is not None else 0, n, off.size - 1, off.ctypes.data,
                                      N.ptr(pack.weights), pack.y_dim, N.ptr(eps), N.ptr(mu), N.ptr(log_var), N.ptr(z), N.ptr(Z), ntot,
                                      col.ctypes.data if col is not None else None, N.ptr(tables_dev) if Z is not None else None, N.stream()),
                "dvae_encode_batch")


def _source(op, spec_or_rows, counts):
    """(src, counts) of what classify_batch accepts: a SpecBatch in layout 1 or 2, a FrameBatch, or strided power rows."""
    if isinstance(spec_or_rows, STFT.SpecBatch):
        if spec_or_rows.layout not in (1, 2):
            raise TypeError(f"{op}: a SpecBatch of power frames (layout 1) or complex frames (layout 2) is required")
        src, counts = spec_or_rows.frames, spec_or_rows.counts
        if not (src.is_cuda and src.dim() == 2 and src.shape[1] == F_BINS and src.dtype == (torch.complex64 if spec_or_rows.layout == 2 else torch.float32)):
            raise TypeError(f"{op}: the SpecBatch's frames must be [sum T_u, 513] on the device, complex64 (layout 2) or float32 (layout 1)")
        return (src.contiguous() if spec_or_rows.layout == 2 else _rows(op, src, "frames", F_BINS)), counts
    if isinstance(spec_or_rows, TGT.FrameBatch):
        spec_or_rows, counts = spec_or_rows.X, spec_or_rows.counts
    src = _rows(op, spec_or_rows, "rows", F_BINS)
    return src, ([src.shape[0]] if counts is None else counts)


def _labels(op, labels, use, y_dim, counts):
    """Label rows [N, y_dim] of a LabelBatch (its `use` labels), a FrameBatch (its Y) or rows."""
    if isinstance(labels, LabelBatch):
        if use not in ("hard", "soft"):
            raise ValueError(f"{op}: use 'hard' or 'soft', got {use!r}")
        y, c = getattr(labels, use), labels.counts
    elif isinstance(labels, TGT.FrameBatch):
        y, c = labels.Y, labels.counts
    else:
        y, c = (labels[:, None] if torch.is_tensor(labels) and labels.dim() == 1 else labels), None
    if c is not None and list(c) != list(counts):
        bad = next((u for u, (a, b) in enumerate(zip(c, counts)) if a != b), min(len(c), len(counts)))
        raise ValueError(f"{op}: utterance {bad}: the labels' frame counts differ from the frames' ({len(c)} and {len(counts)} utterances)")
    return _rows(op, y, "labels", y_dim)


def encode_batch(encoder_or_pack, spec_or_rows, labels=None, counts=None, eps=None, use="hard", y_dim=None):
    """The encoder's latents for every frame of a ragged batch -> LatentBatch.

    encoder_or_pack: an Encoder on the device (packed here; its label width is y_dim if given, else the labels' width, else 0) or
    its EncoderPack of either kind (pack once, encode many batches; pack_encoder picks the kernel).  spec_or_rows: what
    classify_batch accepts -- a SpecBatch of complex frames (layout 2: |X|^2 is formed in the kernel, McemBatch.X2's bits) or of
    power frames (layout 1); a FrameBatch (its X rows); or float32 CUDA power rows [N, 513] (any row stride >= 513) with counts,
    the frames of each utterance laid end to end from row 0 (counts=None: one utterance of all rows).  labels (exactly for
    an encoder that takes them): a LabelBatch (its `use` labels, "hard" or "soft"), a FrameBatch (its Y) or
    float32 CUDA rows [N, y_dim].  eps: float32 CUDA rows [N, z_dim]; with it z = mu + exp(log_var / 2) eps is formed.  TypeError
    naming the shape for an encoder the kernel does not cover; ValueError naming the utterance for tables that do not fit."""
    op = "encode_batch"
    src, counts = _source(op, spec_or_rows, counts)
    if isinstance(encoder_or_pack, EncoderPack):
        pack = encoder_or_pack
    else:
        if y_dim is None:
            y_dim = 0 if labels is None else (labels.y_dim if isinstance(labels, LabelBatch) else labels.Y.shape[1] if isinstance(labels, TGT.FrameBatch)
                                              else 1 if labels.dim() == 1 else labels.shape[1])
        pack = EncoderPack(encoder_or_pack, y_dim)
    off = frame_table(op, counts, src.shape[0])
    if pack.weights.device != src.device:
        raise ValueError(f"{op}: the encoder lives on {pack.weights.device}, the frames on {src.device}")
    if (labels is None) != (pack.y_dim == 0):
        raise ValueError(f"{op}: labels are needed exactly when the encoder takes them (y_dim {pack.y_dim})")
    y = _labels(op, labels, use, pack.y_dim, counts) if labels is not None else None
    if y is not None and y.shape[0] != src.shape[0]:
        raise ValueError(f"{op}: {y.shape[0]} label rows for {src.shape[0]} frames")
    if eps is not None:
        eps = _rows(op, eps, "eps", pack.z_dim).contiguous()
    mu, log_var = (torch.empty((src.shape[0], pack.z_dim), dtype=torch.float32, device=src.device) for _ in range(2))
    z = torch.empty_like(mu) if eps is not None else None
    encode_rows(pack, src, off, y, eps, mu, log_var, z)
    return LatentBatch(mu, log_var, z, counts, off)


def reconstruct_batch(vae, spec_or_rows, labels=None, eps=None, counts=None, use="hard", decode_labels=None, precision="fp32", encoder_pack=None):
    """Encode, then decode (scripts/reconstruct_ntcd_M2.py:231-358: `_, z, _ = model.encoder(x)`, `model.decoder(z | y)` under the
    oracle label, all ones, all zeros) -> (variance [513, N], LatentBatch).  vae: a packages.models VAE (encoder / decoder); the
    encoder takes the labels exactly when its first layer is wider than 513, the decoder when its is wider than 16.  Decodes z, or
    mu when eps is None, with DecoderPack.decode (R = 1) under decode_labels (rows [N, y_dim], a LabelBatch or a FrameBatch;
    default: `labels`).  Utterance u is variance[:, frame_off[u] : frame_off[u + 1]], (513, T_u) as the scripts plot it.
    encoder_pack: an EncoderPack of vae.encoder (either kind, e.g. from pack_encoder): the encoding runs on it and the decoder's input
    is split at its z_dim, so a model of any covered size is reconstructed (DecoderPack picks the generic chain's decode)."""
    from .mcem import DecoderPack
    op = "reconstruct_batch"
    enc_y = vae.encoder.hidden[0].in_features - F_BINS
    if encoder_pack is not None:
        if encoder_pack.y_dim != enc_y:
            raise ValueError(f"{op}: the encoder pack takes {encoder_pack.y_dim} label columns, vae.encoder {enc_y}")
        dec_y = vae.decoder.hidden[0].in_features - encoder_pack.z_dim
        if dec_y < 0:
            raise ValueError(f"{op}: the encoder pack's z_dim {encoder_pack.z_dim} exceeds the decoder's input width")
        lat = encode_batch(encoder_pack, spec_or_rows, labels if enc_y > 0 else None, counts, eps, use)
    else:
        dec_y = vae.decoder.hidden[0].in_features - Z_DIM
        lat = encode_batch(vae.encoder, spec_or_rows, labels if enc_y > 0 else None, counts, eps, use, y_dim=enc_y)
    dl = labels if decode_labels is None else decode_labels
    if (dec_y > 0) != (dl is not None):
        raise ValueError(f"{op}: the decoder takes {dec_y} label columns: labels are needed exactly then")
    zs = (lat.z if eps is not None else lat.mu)[:, None, :]                       # (N, R = 1, 16)
    y = _labels(op, dl, use, dec_y, lat.counts).T.contiguous() if dec_y > 0 else None      # (y_dim, N), the decoder kernels' layout
    var = DecoderPack(vae.decoder, dec_y, precision).decode(zs, y)[0]
    return var, lat
