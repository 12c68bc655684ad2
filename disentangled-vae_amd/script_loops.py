"""The loop bodies of the reference's two M2_info scripts as functions on the drop-in `DeepGenerativeModel_v5`, for
examples/train_script_loop.py, tools/bench_module_info.py and tests/test_gpu_module_info.py: every line is a module call, a loss of
packages/models/utils.py or a stock torch.optim.Adam call, as in the scripts.

    decoder_label "truth"       scripts/training_M2_info_vad.py:159-198           r, z, mu, logvar = model(x, y)
    decoder_label "classifier"  scripts/training_M2_info_vad_pretrain.py:162-200  r, z, mu, logvar = model(x, model.classify_fromX(x)): the label
                                input of the body carries a gradient, and the reconstruction loss trains the classifier through it
    aux_enc "bce" | "uniform" | "entropy"   the adversarial term on the encoder: binary_cross_entropy(aux(z), y), binary_cross_entropy_v2 or
                                binary_cross_entropy_v3 of aux(z) (the pretrain script uses the last, with gamma = beta)
Which kernels a `model(x, y)` call runs on is the module's own affair (module_path.set_info_body / DVAE_MODULE_INFO_BODY).
"""
from packages.models.utils import binary_cross_entropy, binary_cross_entropy_v2, binary_cross_entropy_v3, elbo

DECODER_LABELS = ("truth", "classifier")
AUX_ENCS = ("bce", "uniform", "entropy")


def info_losses(model, x, y, decoder_label="truth", aux_enc="bce", alpha=0.0, beta=10.0, gamma=1.0, eps=1e-8):
    """One forward of the loop body -> dict(ELBO, recon, KL, classif_loss, aux_enc_loss, enc_loss, aux_loss) of 0-dim tensors."""
    if decoder_label not in DECODER_LABELS or aux_enc not in AUX_ENCS:
        raise ValueError(f"decoder_label {decoder_label!r} / aux_enc {aux_enc!r}: the choices are {DECODER_LABELS} and {AUX_ENCS}")
    y_hat_class_soft = model.classify_fromX(x)
    r, z, mu, logvar = model(x, y_hat_class_soft if decoder_label == "classifier" else y)
    ELBO, recon, KL = elbo(x, r, mu, logvar, eps)
    classif_loss = alpha * binary_cross_entropy(y_hat_class_soft, y, eps)
    y_hat_aux_soft = model.classify_fromZ(z)                 # the encoder is trained NOT to let y be predicted from z
    if aux_enc == "bce":
        aux_enc_loss = beta * binary_cross_entropy(y_hat_aux_soft, y, eps)
    elif aux_enc == "uniform":
        aux_enc_loss = beta * binary_cross_entropy_v2(y_hat_aux_soft, eps)
    else:
        aux_enc_loss = beta * binary_cross_entropy_v3(y_hat_aux_soft, eps)
    enc_loss = ELBO + classif_loss - aux_enc_loss
    aux_loss = gamma * binary_cross_entropy(model.classify_fromZ(z.detach()), y, eps)        # the auxiliary net alone learns to predict it
    return dict(ELBO=ELBO, recon=recon, KL=KL, classif_loss=classif_loss, aux_enc_loss=aux_enc_loss, enc_loss=enc_loss, aux_loss=aux_loss)


def info_step(model, opt_body, opt_aux, x, y, **kw):
    """One iteration: info_losses, then the two backward / step / zero_grad triples in the scripts' order.  opt_body: the Adam over
    model.enc_dec_clf.parameters(), opt_aux: the one over model.auxiliary.parameters().  -> the losses (detached)."""
    L = info_losses(model, x, y, **kw)
    L["enc_loss"].backward()
    opt_body.step()
    opt_body.zero_grad()
    L["aux_loss"].backward()
    opt_aux.step()
    opt_aux.zero_grad()
    return {k: v.detach() for k, v in L.items()}
