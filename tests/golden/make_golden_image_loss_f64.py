"""Generates tests/golden/ref_image_loss_f64.npz: the REFERENCE's own `Trainer.calc_dr_loss`
(/root/reference/DSS/training/trainer.py:332-372, with `L1Loss` / `IouLoss` / `BaseLoss` of losses.py and `eps_denom` of
mathHelper.py), unmodified, called unbound as in make_golden_image_loss.py but on FLOAT64 tensors, with autograd providing
the gradients w.r.t. the predicted image and mask.  It ties the float64 yardstick of tests/image_loss_reference.py to the
reference (tests/test_image_loss_reference_cpu.py: 1e-12 of the entry's magnitude).

The inputs are the float32 values of `image_loss_reference.golden_case()` widened to float64: soft masks and soft predicted
alphas in [0, 1] with exact zeros and ones mixed in, exact colour and alpha ties, an image without any target silhouette, an
all-empty image (U == 0) and an image whose masks are of order 1e-18 on a few pixels (0 < U < 1e-17, t > 0: the clamped branch
of `eps_denom` with a non-zero gradient).  Two weightings: configs/dss.yml's (1, 1) and (0.7, 2.0) as fp32 holds them.

    python tests/golden/make_golden_image_loss_f64.py
"""
import os
import sys
import types

import numpy as np
import torch

import make_golden_image_loss as g32  # (installs the stubs, imports the unmodified reference modules)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_loss_reference as ir  # noqa: E402


def run(c, lam_rgb, lam_sil):
    fake = types.SimpleNamespace(lambda_dr_silhouette=lam_sil, lambda_dr_rgb=lam_rgb,
                                 l1_loss=g32.ref_losses.L1Loss(reduction="mean"),
                                 iou_loss=g32.ref_losses.IouLoss(reduction="mean", channel_dim=None))
    t_pred = torch.from_numpy(c.rgba[..., :3].astype(np.float64)).requires_grad_(True)
    t_mp = torch.from_numpy(c.rgba[..., 3].astype(np.float64)).requires_grad_(True)
    loss = {"loss": 0}
    g32.ref_trainer.Trainer.calc_dr_loss(fake, torch.from_numpy(c.img.astype(np.float64)), t_pred,
                                         torch.from_numpy(c.mask.astype(np.float64)), t_mp, reduction_method="mean", loss=loss)
    assert loss["loss"].dtype == torch.float64
    loss["loss"].backward()
    val = {k: (v.item() if torch.is_tensor(v) else float(v)) for k, v in loss.items()}
    grad = np.concatenate([t_pred.grad.numpy(), t_mp.grad.numpy()[..., None]], -1)
    return np.array([val["loss"], val["loss_dr_rgb"], val["loss_dr_silhouette"]], np.float64), grad


def main():
    c = ir.golden_case()
    out = {"rgba": c.rgba, "img": c.img, "mask": c.mask}
    for tag, lam in zip("ab", ir.LAMBDAS):
        out[tag + "_lambdas"] = np.array(lam, np.float64)
        out[tag + "_losses"], out[tag + "_grad"] = run(c, *lam)
        print(tag, lam, out[tag + "_losses"])
    path = os.path.join(HERE, "ref_image_loss_f64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
