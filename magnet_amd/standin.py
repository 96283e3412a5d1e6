"""Deterministic stand-ins for the backbones this build does not contain (the D-Net needs torch.hub and
its checkpoint; the F-Net has a matrix-core implementation in magnet_amd/fnet.py but no weights offline): tiny seeded
modules with the backbones' output contracts, the argparse fields `MAGNET.__init__` reads, and seeded g_net / mask_head
weights.  Used by the synthetic evaluation driver (eval_synthetic.py), `__graft_entry__.smoke()` and the tests — the golden
generator drives the REFERENCE `MAGNET.forward` with the same stand-ins, so both sides see identical (mu, sigma, x_d3,
features)."""
from types import SimpleNamespace

import torch
import torch.nn as nn


class StubDNet(nn.Module):
    """img (N,3,H,W) -> ((N,2,H/4,W/4) [mu, sigma>0], (N,256,H/4,W/4)) like DNET(dnet=False)
    (reference: models/DNET.py:62-67, submodules/D_dense_depth.py:187-195)."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.head = nn.Conv2d(3, 2, 4, stride=4)
        self.feat = nn.Conv2d(3, 256, 4, stride=4)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)

    def forward(self, img):
        o = self.head(img)
        mu = 1.0 + 3.0 * torch.sigmoid(o[:, 0:1])
        sigma = 0.05 + 0.3 * torch.sigmoid(o[:, 1:2])
        return torch.cat([mu, sigma], dim=1), self.feat(img)


class StubFNet(nn.Module):
    """img (N,3,H,W) -> (N,fdim,H/4,W/4) linear signed features like FNET (models/FNET.py:19-20)."""

    def __init__(self, seed=0, fdim=64):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv = nn.Conv2d(3, fdim, 4, stride=4)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.7)

    def forward(self, img):
        return self.conv(img)


def make_args(D=5, iters=3, dpv_h=120, dpv_w=160, beta=3, weighting="CW5", fdim=64, V=4):
    """The argparse fields MAGNET.__init__ reads (reference: models/MAGNET.py:95-104,
    test_MaGNet.py:89-147)."""
    return SimpleNamespace(
        MAGNET_sampling_range=beta, MAGNET_num_samples=D, MAGNET_mvs_weighting=weighting,
        MAGNET_num_train_iter=iters, MAGNET_num_test_iter=iters, MAGNET_num_source_views=V,
        dpv_height=dpv_h, dpv_width=dpv_w, downsample_ratio=4, FNET_feature_dim=fdim,
        DNET_ckpt=None, FNET_ckpt=None, MAGNET_ckpt=None)


def seeded_magnet_weights(model, seed=0, gain=1.0):
    """Deterministic g_net / mask_head weights (same draw order for the reference module and ours:
    both expose `g_net.gnet.{0,2,4,6}` and `mask_head.{0,2,4,6}`); `gain` scales every tensor (the training-step vector
    uses 0.25 so that sigma stays away from the loss's variance clamp)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in (model.g_net, model.mask_head):
            for name, p in sorted(mod.state_dict().items()):
                scale = 0.05 if p.dim() > 1 else 0.01
                p.copy_(torch.randn(p.shape, generator=g) * (scale * gain))


class StandinEncoder(nn.Module):
    """A cheap seeded stand-in for the D-Net's EfficientNet-B5 encoder (reference: models/submodules/D_dense_depth.py:7-25): img
    (N,3,H,W) -> the reference's 12-entry feature list with B5's shapes where the decoder reads: [4] 24 channels at 1/2, [5] 40 at 1/4,
    [6] 64 at 1/8, [8] 176 at 1/16, [11] 2048 at 1/32 (each stride-2 stage rounds up, as B5's 'same' padding does).  Each map is a
    seeded 3x3 convolution of the average-pooled image followed by SiLU; entry 0 is the image, the entries no decoder reads are None."""

    STAGES = ((4, 1, 24), (5, 2, 40), (6, 3, 64), (8, 4, 176), (11, 5, 2048))      # (index, number of 2x poolings, channels)

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.convs = nn.ModuleList(nn.Conv2d(3, c, 3, padding=1) for _, _, c in self.STAGES)
        with torch.no_grad():
            for conv in self.convs:
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 1.5)
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.3)

    def forward(self, img):
        feats = [img] + [None] * 11
        x, done = img, 0
        for (idx, n_pool, _), conv in zip(self.STAGES, self.convs):
            while done < n_pool:
                x = nn.functional.avg_pool2d(x, 2, 2, ceil_mode=True)
                done += 1
            feats[idx] = nn.functional.silu(conv(x))
        return feats


def make_dnet_args(downsample_ratio=4):
    """The argparse fields of the reference's DNET (models/DNET.py:8-33) for MaGNet's D-Net."""
    return SimpleNamespace(output_type="G", DNET_architecture="DenseDepth_BN", output_dim=2, downsample_ratio=downsample_ratio,
                           DNET_fix_encoder_weights="None")


def make_dnet(seed=0, enc_seed=0, depth_prior=True, dnet=False, backend="torch", split_k=0, precision="bf16x3", encoder="standin",
              encoder_backend="torch", encoder_precision="bf16x3"):
    """magnet_amd.dnet.DNET with the stand-in encoder and seeded decoder weights (magnet_amd.dnet.seeded_decoder_state), in eval mode.
    encoder: "standin" (default: StandinEncoder(enc_seed)) or "b5": magnet_amd.encoder.Encoder(backend=encoder_backend), the real
    EfficientNet-B5 with calibrated seeded weights (magnet_amd.encoder.load_seeded_encoder(enc_seed)).
    encoder_precision: EncoderMFMA's format, "bf16x3" (default) or "fp16" (reduced precision, opt-in); "fp16" goes with encoder="b5" and
    encoder_backend="hip".
    dnet=False: MaGNet's D-Net; dnet=True: the stand-alone D-Net (img -> (N, 2, H, W) [mu, variance]); backend, split_k, precision: see DNET.
    depth_prior: the depth head's last layer is scaled by 1/4 and its bias set to (2.5, -3) so that the stand-in predicts
    plausible scenes for the matcher, mu around 2.5 m (+-1.5) and sigma around 0.2 m (StubDNet's ranges); the raw recipe's mu is
    centred on zero, where depth candidates cross the camera plane."""
    from .dnet import DNET, load_seeded_decoder
    if encoder_precision != "bf16x3" and not (encoder == "b5" and encoder_backend == "hip"):
        raise ValueError(f"make_dnet: encoder_precision={encoder_precision!r} goes with encoder='b5' and encoder_backend='hip' (a mode of EncoderMFMA)")
    if encoder == "b5":
        from .encoder import Encoder, load_seeded_encoder
        enc = load_seeded_encoder(Encoder(backend=encoder_backend, precision=encoder_precision), enc_seed)
    elif encoder == "standin":
        if encoder_backend != "torch":
            raise ValueError("make_dnet: encoder_backend='hip' goes with encoder='b5' (the stand-in is a torch module)")
        enc = StandinEncoder(enc_seed)
    else:
        raise ValueError(f"make_dnet: encoder must be 'standin' or 'b5', got {encoder!r}")
    d = DNET(make_dnet_args(), enc, dnet=dnet, backend=backend, split_k=split_k, precision=precision)
    load_seeded_decoder(d.d_net.decoder, seed)
    if depth_prior:
        with torch.no_grad():
            d.d_net.decoder.depth_head[4].weight.mul_(0.25)
            d.d_net.decoder.depth_head[4].bias.copy_(torch.tensor([2.5, -3.0]))
    return d.eval()
