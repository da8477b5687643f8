"""Batched multi-sample validation: what the reference does one image and
one sample at a time (`for val_data: for k in range(cfg.sample): model.test_val(...)`,
lib/trainer_temp.py:441-446 -> model/sr3d/model.py:368-375,428-433) as ONE sharded batch of
images x samples through the HIP sampler, followed by the PSNR / SSIM of core/metrics.py.

SSIM restates core/metrics.py:84-104 with numpy only: `cv2.filter2D(img, -1, window)[5:-5, 5:-5]`
with an 11x11 window is exactly the 'valid' correlation with that window, and
`cv2.getGaussianKernel(11, 1.5)` is the normalised exp(-(i-5)^2 / (2*1.5^2)). cv2 is not available
in the build container, so this file's SSIM is checked against an independent scipy evaluation,
not against cv2 itself (parity unpinned for the cv2 call, formula-level faithful).

The host functions are the default and the yardstick. `validate_batch(metrics="device")` / `device_scores` compute the
same scores on the device (sr3_metrics_psnr_ssim, csrc/kernels_metrics.hip) so that only two numbers per image leave it.

`loss_by_level` is the checkpoint diagnostic: the denoising loss of a set of images over noise levels, one batch of
images x levels through sr3_denoise_loss.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from .metrics import psnr, tensor2img


def gaussian_kernel(ksize: int = 11, sigma: float = 1.5) -> np.ndarray:
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return k / k.sum()


def _valid_filter(img: np.ndarray, k1: np.ndarray) -> np.ndarray:
    # separable 'valid' correlation (the window is an outer product of a symmetric kernel)
    n = k1.size
    h = sum(k1[j] * img[:, j:img.shape[1] - n + 1 + j] for j in range(n))
    return sum(k1[j] * h[j:h.shape[0] - n + 1 + j, :] for j in range(n))


def ssim(img1: np.ndarray, img2: np.ndarray) -> float:
    """core/metrics.py:84-104 for one 2-D image pair in [0, 255]."""
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    k = gaussian_kernel(11, 1.5)
    mu1, mu2 = _valid_filter(a, k), _valid_filter(b, k)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _valid_filter(a * a, k) - mu1_sq
    s2 = _valid_filter(b * b, k) - mu2_sq
    s12 = _valid_filter(a * b, k) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return float(m.mean())


def calculate_ssim(img1: np.ndarray, img2: np.ndarray) -> float:
    """core/metrics.py:107-125. For HxWx3 input the reference averages three evaluations of
    `ssim(img1, img2)` on the WHOLE 3-channel arrays (it never indexes the channel); filter2D treats
    channels independently, so that equals the mean of the per-channel SSIM maps — computed so here."""
    if img1.shape != img2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if img1.ndim == 2:
        return ssim(img1, img2)
    if img1.ndim == 3:
        if img1.shape[2] == 3:
            return float(np.mean([ssim(img1[..., c], img2[..., c]) for c in range(3)]))
        if img1.shape[2] == 1:
            return ssim(np.squeeze(img1), np.squeeze(img2))
    raise ValueError("Wrong input image dimensions.")


def scores_from_sums(ssd, n_values: int) -> np.ndarray:
    """PSNR (core/metrics.py:74-81) from exact sums of squared uint8 differences over `n_values` values each:
    20*log10(255/sqrt(ssd/n)), inf where ssd == 0. Bit-equal to `metrics.psnr` on the same images: a sum of integer
    squares below 2^53 is exact in float64 whatever the order, and the rest is the same libm calls."""
    ssd = np.asarray(ssd)
    out = np.empty(ssd.shape, dtype=np.float64)
    flat = out.reshape(-1)
    for j, v in enumerate(ssd.reshape(-1)):
        mse = float(np.float64(int(v)) / np.float64(int(n_values)))
        flat[j] = math.inf if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))
    return out


def device_scores(netG, images: "torch.Tensor", hr: "torch.Tensor", row_offset: int = 0) -> Dict[str, np.ndarray]:
    """PSNR / SSIM of `images` [B,3,H,W] (CUDA, any range) against `hr` [N,3,H,W] (CUDA) on the device
    (sr3_metrics_psnr_ssim): row b is scored against hr[(row_offset + b) % N], so `hr` is never replicated. Same scores as
    `metrics.psnr` / `calculate_ssim` on `metrics.tensor2img` of both (PSNR bit-equal, SSIM to ~1e-14). Only the 2 x B
    results cross to the host. Returns {"psnr": float64 [B], "ssim": float64 [B]} (numpy)."""
    import torch
    from .postprocess import _check, _unet

    sr, hr = _check(images), _check(hr)
    if hr.device != sr.device or hr.shape[2:] != sr.shape[2:]:
        raise RuntimeError(f"images {tuple(sr.shape)} on {sr.device} and hr {tuple(hr.shape)} on {hr.device} do not match")
    B, _, H, W = sr.shape
    ssd = torch.empty(B, dtype=torch.int64, device=sr.device)
    ss = torch.empty(B, dtype=torch.float64, device=sr.device)
    unet = _unet(netG)
    eng = unet.engine()
    unet.ready()
    eng.metrics(sr.data_ptr(), hr.data_ptr(), B, hr.shape[0], int(row_offset), H, W, ssd.data_ptr(), ss.data_ptr())
    unet.finish()
    return {"psnr": scores_from_sums(ssd.cpu().numpy(), 3 * H * W), "ssim": ss.cpu().numpy()}


def lr_consistency(netG, images: "torch.Tensor", lr, row_offset: int = 0) -> Dict[str, np.ndarray]:
    """How far `images` [B,3,H,W] (CUDA) are from downsampling to their low-resolution inputs, on the device
    (sr3_lr_residual): row b is scored against lr[(row_offset + b) % N] (fp32 [N,3,l,l] in [-1,1] or uint8 [N,l,l,3]) under
    the reference's degradation in real arithmetic, A = the antialiased bicubic resample. Needs no HR
    image: the SR3 paper's "consistency". Returns {"mse": float64 [B] mean squared residual, "max_abs": float32 [B]}."""
    import torch
    from .diffusion import lr_to_tensor
    from .postprocess import _check, _unet

    img = _check(images)
    y = lr_to_tensor(lr).to(img.device)
    B, C, H, W = img.shape
    N, Cl, lh, lw = y.shape
    if Cl != C or lh >= H or lw >= W:
        raise RuntimeError(f"images {tuple(img.shape)} and lr {tuple(y.shape)} do not match")
    ss = torch.empty(B, dtype=torch.float64, device=img.device)
    mx = torch.empty(B, dtype=torch.float32, device=img.device)
    unet = _unet(netG)
    eng = unet.engine()
    unet.ready()
    eng.lr_residual(img.data_ptr(), B, C, H, W, y.data_ptr(), N, lh, lw, int(row_offset), ss.data_ptr(), mx.data_ptr())
    unet.finish()
    return {"mse": ss.cpu().numpy() / float(C * lh * lw), "max_abs": mx.cpu().numpy()}


def _gather_rows(local: "torch.Tensor", n_total: int, gpu: "torch.device") -> "torch.Tensor":
    """dist.all_gather_images for a tensor on any device: the collective runs where the backend has one — host memory
    for gloo, the rank's GPU `gpu` for nccl (RCCL) — and the result comes back on `local`'s device."""
    import torch
    from . import dist as _dist
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return local
    where = torch.device("cpu") if torch.distributed.get_backend() == "gloo" else gpu
    return _dist.all_gather_images(local.to(where), n_total).to(local.device)


def validate_batch(netG, sr: "torch.Tensor", hr: "torch.Tensor", samples: int = 1,
                   seed: Optional[int] = None, sharded: bool = False, metrics: str = "host",
                   keep_images: bool = True, lr=None) -> Dict[str, np.ndarray]:
    """Runs `samples` independent SR3 chains per conditioning image as one batch of N*samples
    images (sample k of image i is batch row k*N + i) and scores them against `hr`.

    sr, hr: [N,3,r,r] in [-1,1] (the dataset's 'SR' and 'HR' entries, datasets/LRHR_dataset.py:93-99).
    N * samples may exceed what one library call takes (~250 images at 128x128): `sample_batch` runs equal chunks
    with the Philox streams keyed by the global row, so the noise does not depend on the chunking. By default the images
    do, within fp32 round-off in f32 / f16x3 and up to about 1e-4 in f16f8 (the chunk size decides which convs take the
    fp8 products); under netG.set_batch_invariant() images and scores are bit-equal whatever the chunking.
    The chains use netG's sampler setting (GaussianDiffusion.set_sampler: the reference's DDPM loop by default).
    Under a warm start (GaussianDiffusion.set_start) every chain starts from its own row of `sr`, noised with its own
    Philox stream, and runs netG.num_steps_run steps.
    Returns per (sample, image) PSNR / SSIM arrays and their means. The reference's running
    `avg / idx * sample` (lib/trainer_temp.py:445-446) multiplies by `sample` instead of dividing —
    the plain means are reported here.

    metrics="host" (default): every image is copied to the host and scored there (metrics.psnr, calculate_ssim).
    metrics="device": the images are scored where they are (device_scores); with sharded=True every rank scores its
    own shard (dist.shard_bounds; a rank left without rows samples nothing) and the ranks exchange the two score
    arrays — on the GPU with nccl / RCCL, through host memory with gloo; the images are gathered only if keep_images.
    keep_images=False: "images" is None in the result.

    lr (fp32 [N,3,l,l] in [-1,1] or uint8 [N,l,l,3]): adds "consistency" ([samples, N] mean squared residual of every
    sample against its LR image, lr_consistency) and "mean_consistency". That score needs no HR image: with lr given, hr
    may be None, and "psnr" / "ssim" and their means are then None. Whether the chains are PROJECTED onto their LR images
    is netG's setting (GaussianDiffusion.set_lr_consistency), not this argument's.
    """
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    if hr is None and lr is None:
        raise ValueError("validate_batch needs hr (PSNR / SSIM), lr (consistency) or both")
    if lr is not None:
        from .diffusion import lr_to_tensor
        lr = lr_to_tensor(lr)
        if lr.shape[0] != sr.shape[0]:
            raise ValueError(f"lr holds {lr.shape[0]} images, sr {sr.shape[0]}")
    if hr is None:
        return _validate_lr_only(netG, sr, lr, samples, seed, sharded, keep_images)
    import torch
    from . import dist as _dist

    N = sr.shape[0]
    x = sr.repeat(samples, 1, 1, 1)
    if seed is None:
        seed = netG._draw_seed()
        if sharded and torch.distributed.is_available() and torch.distributed.is_initialized():
            # every rank must key the Philox streams with the SAME seed (image i's stream does not
            # depend on the world size, dist.py): rank 0's draw wins
            box = [seed]
            torch.distributed.broadcast_object_list(box, src=0)
            seed = int(box[0])
    if metrics == "device":
        a, b = 0, samples * N
        if sharded and torch.distributed.is_available() and torch.distributed.is_initialized():
            a, b = _dist.shard_bounds(samples * N, torch.distributed.get_world_size(), torch.distributed.get_rank())
        if b > a:
            out = netG.super_resolution_batch(x[a:b], seed=seed, image_offset=a)
            sc = device_scores(netG, out, hr.to(out.device), row_offset=a)
        else:       # more ranks than rows: this rank has nothing to sample and contributes nothing to the gather
            out = torch.empty((0,) + tuple(x.shape[1:]), dtype=torch.float32, device=next(netG.parameters()).device)
            sc = {"psnr": np.empty(0), "ssim": np.empty(0)}
        if sharded:
            both = _gather_rows(torch.from_numpy(np.stack([sc["psnr"], sc["ssim"]], axis=1)), samples * N, out.device).numpy()
            sc = {"psnr": both[:, 0], "ssim": both[:, 1]}
            out = _gather_rows(out, samples * N, out.device) if keep_images else None
        ps, ss = sc["psnr"].reshape(samples, N).copy(), sc["ssim"].reshape(samples, N).copy()
    else:
        if sharded:
            out = _dist.sharded_super_resolution(
                lambda xs, off: netG.super_resolution_batch(xs, seed=seed, image_offset=off), x)
        else:
            out = netG.super_resolution_batch(x, seed=seed)
        out_np, hr_np = out.float().cpu().numpy(), hr.float().cpu().numpy()
        ps = np.zeros((samples, N)); ss = np.zeros((samples, N))
        for k in range(samples):
            for i in range(N):
                a, b = tensor2img(out_np[k * N + i]), tensor2img(hr_np[i])
                ps[k, i] = psnr(a, b)
                ss[k, i] = calculate_ssim(a, b)
    finite = np.isfinite(ps)
    res = {"psnr": ps, "ssim": ss, "images": out if keep_images else None,
           "mean_psnr": float(ps[finite].mean()) if finite.any() else math.inf,
           "mean_ssim": float(ss.mean())}
    if lr is not None:
        if out is None or out.shape[0] != samples * N:      # device metrics, sharded, images not gathered
            raise ValueError("validate_batch(lr=...) scores the gathered images: with sharded device metrics keep_images must be True")
        dev = next(netG.parameters()).device
        cons = lr_consistency(netG, out.to(dev), lr)["mse"].reshape(samples, N)
        res["consistency"], res["mean_consistency"] = cons, float(cons.mean())
    return res


def _validate_lr_only(netG, sr, lr, samples, seed, sharded, keep_images):
    """validate_batch without HR: the chains and their consistency score only."""
    import torch
    from . import dist as _dist

    N = sr.shape[0]
    x = sr.repeat(samples, 1, 1, 1)
    if seed is None:
        seed = netG._draw_seed()
        if sharded and torch.distributed.is_available() and torch.distributed.is_initialized():
            box = [seed]
            torch.distributed.broadcast_object_list(box, src=0)
            seed = int(box[0])
    if sharded:
        out = _dist.sharded_super_resolution(lambda xs, off: netG.super_resolution_batch(xs, seed=seed, image_offset=off), x)
    else:
        out = netG.super_resolution_batch(x, seed=seed)
    cons = lr_consistency(netG, out.to(next(netG.parameters()).device), lr)["mse"].reshape(samples, N)
    return {"psnr": None, "ssim": None, "mean_psnr": None, "mean_ssim": None, "images": out if keep_images else None,
            "consistency": cons, "mean_consistency": float(cons.mean())}


def loss_by_level(netG, hr: "torch.Tensor", sr: "torch.Tensor", levels, noise: "Optional[torch.Tensor]" = None,
                  seed: Optional[int] = None, max_chunk: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The denoising loss (GaussianDiffusion.p_losses, evaluation only) of N images at K noise levels: the curve that
    shows whether a checkpoint was ingested correctly and whether an arithmetic mode changes the network's prediction.

    hr, sr: [N,3,H,W] on the GPU (sr is ignored by an unconditional model). levels: a sequence of K values of
    sqrt(alpha_cumprod) in [0, 1], or an int K = that many entries of sqrt_alphas_cumprod_prev[1:], evenly spaced by index
    (first and last included). netG.set_loss() selects l1 / l2. The K x N evaluations run as ONE batch (level k of image i
    is row k*N + i; chunked above the per-call limit, max_chunk lowers it); hr and sr are indexed with % N, never
    replicated. Every image meets the SAME noise at every level, so the curve of an image moves with the level alone:
    noise [N,3,H,W] is indexed by the source image, and with noise=None the Philox stream is keyed by the source image
    (seed, i) — not by the row — under `seed` (None: a fresh one).

    Returns {"levels": fp32 [K], "loss": [K] mean loss per element (the sum over the N images / (N*3*H*W)),
    "per_image": fp64 [K,N] summed loss of every image}."""
    import torch

    hr, sr = netG._loss_inputs({"HR": hr, "SR": sr})
    N, C, H, W = hr.shape
    if isinstance(levels, (int, np.integer)):
        prev = np.asarray(netG.sqrt_alphas_cumprod_prev, dtype=np.float64)[1:]
        if not 1 <= int(levels) <= prev.size:
            raise ValueError(f"levels={levels}: need 1 <= K <= T = {prev.size}")
        levels = prev[np.round(np.linspace(0, prev.size - 1, int(levels))).astype(np.int64)]
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float32).reshape(-1))
    if lv.size < 1 or not (np.isfinite(lv).all() and (lv >= 0).all() and (lv <= 1).all()):
        raise ValueError("levels must be values of sqrt(alpha_cumprod) in [0, 1]")
    if noise is not None:
        noise = noise.to(device=hr.device, dtype=torch.float32).contiguous()
        if tuple(noise.shape) != tuple(hr.shape):
            raise RuntimeError(f"noise must be {tuple(hr.shape)} (one image per source image), got {tuple(noise.shape)}")
    elif seed is None:
        seed = netG._draw_seed()
    res = netG._loss_rows(hr, sr, torch.from_numpy(np.repeat(lv, N)), netG.loss_func, noise=noise, noise_per_source=True,
                          seed=seed or 0, max_chunk=max_chunk)
    per = res["per_image"].cpu().numpy().reshape(lv.size, N)
    return {"levels": lv, "loss": per.sum(axis=1) / float(N * C * H * W), "per_image": per}


def mc_dropout(netG, x_sr: "torch.Tensor", passes: int, noise_seed: int, dropout_seed: int, image_offset: int = 0):
    """Monte-Carlo dropout over the sampler: `passes` (K) calls of netG.sample_batch on the same
    conditioning with the SAME diffusion noise (noise_seed) and K dropout seeds dropout_seed, dropout_seed + 1, ... —
    what varies between the passes is only the masks of the UNet's Dropout, so the spread is the model's own
    uncertainty about each pixel. netG must have opted in (set_dropout_sampling(True)) and be in train() mode;
    otherwise dropout is the identity, every pass is the same image and the std is exactly 0.

    Returns (mean, std): per-pixel mean and population standard deviation (divisor K) over the passes, fp32 [B,C,H,W]
    device tensors; the sum and the sum of squared deviations are formed in fp64 in pass order. The pinned dropout seed of
    netG is restored afterwards."""
    import torch

    if passes < 1:
        raise ValueError("mc_dropout: passes must be >= 1")
    unet = netG.denoise_fn
    keep = unet.dropout_seed
    outs = []
    try:
        for k in range(int(passes)):
            unet.dropout_seed = int(dropout_seed) + k
            outs.append(netG.sample_batch(x_sr, False, None, int(noise_seed), image_offset))
    finally:
        unet.dropout_seed = keep
    stack = torch.stack(outs).to(torch.float64)
    mean = stack.sum(dim=0) / len(outs)
    var = ((stack - mean) ** 2).sum(dim=0) / len(outs)
    return mean.to(torch.float32), var.sqrt().to(torch.float32)
