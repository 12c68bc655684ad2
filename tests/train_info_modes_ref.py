"""The M2_info train step with the two options of the fused step (include/dvae_train.h: dvae_train_info_plan_mode;
disentangled-vae_amd/trainer_info.py: dec_label, aux_enc) in numpy at any dtype: the loop body of
scripts/training_M2_info_vad_pretrain.py:162-200 and its kin, composed from the pieces of oracle/vae_oracle.py.  No GPU here.

    dec_label  "truth": the decoder sees [z | y]; "classifier": [z | clf(x)], and the label columns' gradient of decoder layer 1 joins
               alpha dBCE / d p_c on its way into the classifier;
    aux_enc    V in enc_loss = ELBO + alpha BCE(clf(x), y) - beta V: "bce" BCE(aux(z), y), "uniform" binary_cross_entropy_v2(aux(z)),
               "entropy" binary_cross_entropy_v3(aux(z)); aux_loss = gamma BCE(aux(z.detach()), y) whatever V is.

With the defaults every operation is the one vo.m2info_losses_and_grads performs, in its order, so the results are equal bit for bit
(tests/test_train_info_modes_cpu.py)."""
import numpy as np

from oracle import vae_oracle as vo

DEC_LABELS = ("truth", "classifier")
AUX_ENCS = ("bce", "uniform", "entropy")


def losses_and_grads(params, x, y, eps_noise, alpha, beta, gamma, eps=1e-8, dec_label="truth", aux_enc="bce"):
    """What vo.m2info_losses_and_grads returns: (out, grads after enc_loss.backward(), what aux_loss.backward() adds to the
    auxiliary net's)."""
    if dec_label not in DEC_LABELS or aux_enc not in AUX_ENCS:
        raise ValueError((dec_label, aux_enc))
    pre = "enc_dec_clf."
    clf = vo.classifier_fwd(params, pre + "classifier.", x)
    enc, dec = vo.m2v3_forward(params, x, y if dec_label == "truth" else clf["p"], eps_noise, pre)
    ELBO, recon, kl = vo.elbo(x, dec["r"], enc["mu"], enc["lv"], eps)
    classif_loss = alpha * vo.binary_cross_entropy(clf["p"], y, eps)
    aux1 = vo.classifier_fwd(params, "auxiliary.", enc["z"])
    if aux_enc == "bce":
        V = vo.binary_cross_entropy(aux1["p"], y, eps)
    elif aux_enc == "uniform":
        V = vo.binary_cross_entropy_v2(aux1["p"], eps)
    else:
        V = vo.binary_cross_entropy_v3(aux1["p"], eps)
    aux_enc_loss = beta * V
    enc_loss = ELBO + classif_loss - aux_enc_loss
    aux2 = vo.classifier_fwd(params, "auxiliary.", enc["z"])  # z.detach(): same values
    aux_loss = gamma * vo.binary_cross_entropy(aux2["p"], y, eps)

    g1 = {}
    da, dmu_kl, dlv_kl = vo.elbo_bwd(x, dec["a"], enc["mu"], enc["lv"])
    ddec_in = vo.decoder_bwd(params, g1, pre + "decoder.", dec, da)
    zdim = enc["z"].shape[1]
    dz = ddec_in[:, :zdim]
    # -beta V(aux(z)): into the auxiliary net and into z
    if aux_enc == "bce":
        dp_aux = vo.bce_bwd(aux1["p"], y, eps, -beta)
    elif aux_enc == "uniform":
        dp_aux = vo.bce_v2_bwd(aux1["p"], eps, -beta)
    else:
        dp_aux = vo.bce_v3_bwd(aux1["p"], eps, -beta)
    dz_aux = vo.classifier_bwd(params, g1, "auxiliary.", aux1, dp_aux, need_dx=True)
    dz = dz + dz_aux
    vo.encoder_bwd(params, g1, pre + "encoder.", enc, dz, dmu_kl, dlv_kl, need_dx=False)
    # + alpha BCE(clf(x), y), and what the decoder's label columns hand back when they were fed clf(x)
    dp_clf = vo.bce_bwd(clf["p"], y, eps, alpha)
    if dec_label == "classifier":
        dp_clf = dp_clf + ddec_in[:, zdim:]
    vo.classifier_bwd(params, g1, pre + "classifier.", clf, dp_clf, need_dx=False)

    g2 = {}
    dp_aux2 = vo.bce_bwd(aux2["p"], y, eps, gamma)
    vo.classifier_bwd(params, g2, "auxiliary.", aux2, dp_aux2, need_dx=False)

    out = dict(r=dec["r"], z=enc["z"], mu=enc["mu"], logvar=enc["lv"],
               y_hat_class_soft=clf["p"], y_hat_aux_soft=aux1["p"],
               ELBO=ELBO, recon=recon, kl=kl, classif_loss=classif_loss,
               aux_enc_loss=aux_enc_loss, enc_loss=enc_loss, aux_loss=aux_loss)
    return out, g1, g2


def train_step(params, opt_edc, opt_aux, x, y, eps_noise, alpha=0.0, beta=10.0, gamma=1.0, eps=1e-8, lr=1e-4, dec_label="truth",
               aux_enc="bce"):
    """What vo.train_step_m2info returns: (out, g1, g2, what the auxiliary net is stepped with).  The script never zeroes what
    enc_loss.backward() leaves in the auxiliary net, so that is g1 + g2 = gamma dBCE - beta dV."""
    out, g1, g2 = losses_and_grads(params, x, y, eps_noise, alpha, beta, gamma, eps, dec_label, aux_enc)
    opt_edc.step(params, g1, lr=lr)
    aux_total = {k: g1[k] + g2[k] for k in g2}
    opt_aux.step(params, aux_total, lr=lr)
    return out, g1, g2, aux_total
