"""Drop-in backbone: the reference's ``BaseVAMPIRE2`` module API over the HIP hot path.

Mirrors /root/reference/src/layers/backbones/base_vampire2.py (``bv2``):

* constructor kwargs                                       bv2:83-104
* registered buffers ``frustum, camera_mids, bev_mids, voxel_coords, occ_coords,
  norm_voxel_coords (cat_pos), output_coords`` -- same names, shapes and values, so the
  published checkpoints load                               bv2:146-160
* attributes ``fD fH fW vZ vY vX oY depth_channels``       bv2:148-165
* submodules ``img_backbone img_neck mapping_along_depth channel_lower base_conv
  density_conv seg_conv density rgb_conv voxel_output upsample2d``   bv2:167-210
* ``get_geometry / get_pixel / get_voxel_feats / volume_rendering_from_multiple_views``
  with the reference's signatures and return tuples       bv2:314-516
* ``forward(sweep_imgs, mats_dict, inrange_pts=None, timestamps=None)`` -> the 12-tuple
                                                           bv2:637-693

What differs underneath: the 2D->3D lift and the volume renderer run as hand-written HIP
kernels (``vampire_amd.ops.HotPath``); ``_forward_single_sweep`` feeds the lift with the
depth distribution and the low-channel features directly (the 372 MB outer product of
bv2:553 is never built) and lets the renderer evaluate the frustum geometry in-kernel.
The dense convolutions around the path (image backbone/neck, 3-D UNet, heads) are ordinary
torch modules (MIOpen) and are out of this build's scope; when mmdet / mmdet3d are not
installed a small stand-in encoder keeps the module constructible and runnable.

MIOpen note (measured, tools/time_unet3d.py / tools/time_backbone.py): in fp32 with torch's default
immediate mode the 3x3x3 weight-gradient solver picked for the Unet3D layers takes 53 ms per
layer on gfx950 (660 ms per module backward at cfg-B); with ``torch.backends.cudnn.benchmark =
True`` (MIOpen find) the module backward is 23 ms, and under the reference's AMP it is 12 ms.
Set that flag in the training script; this module does not touch global torch state.
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import geometry as G
from .config import PathConfig
from .density import ModifyLaplaceDensity
from .layers import (HeadSegment, conv3d_3x3x3, conv3d_bf16, conv3d_bf16_stride2, conv3d_fused, conv3d_heads, conv3d_kind,
                     cuda_autocast)
from .ops import HotPath


# ---------------------------------------------------------------------------
# dense layers around the path (plain torch; bv2:17-78)
# ---------------------------------------------------------------------------
def _resize(x, size):
    """F.interpolate(x, size, mode='trilinear', align_corners=True) (bv2:66, 72): the HIP resize for
    device tensors (its backward is a gather; aten's atomic scatter is 8.8 ms of the module's
    backward at cfg-B), torch for CPU tensors like the other dense layers."""
    if x.is_cuda and x.dim() == 5:
        from .layers import upsample_trilinear
        from . import _capi
        # scale factors beyond the backward's gather table (about 6x per axis) go to aten
        if _capi.checked().vamp_upsample_trilinear_supported(*x.shape[2:], *[int(v) for v in size]):
            return upsample_trilinear(x, size)
    return F.interpolate(x, tuple(size), mode="trilinear", align_corners=True)


# Switches of the module path, read ONCE at import (not on every forward): VAMP_CONV3D=0 keeps MIOpen for
# every 3-D convolution, VAMP_CONV3D_MIN_VOXELS is the volume size from which the HIP convolution is
# used, VAMP_GLUE=hip routes the depth softmax / density gate through the standalone HIP kernels,
# VAMP_FUSE=0 turns the fused producer / consumer forms off, VAMP_CONV3D_S2=0 keeps MIOpen for the stride-2 3x3x3
# layers under a 16-bit autocast (default: the HIP kernels of conv3d_bf16_s2.hip), VAMP_RESIZE2D=1 routes the x4
# resize of the three rendered camera maps and the 256-cell grid's 0.5x resize through resize2d.hip (default: aten),
# VAMP_QUERIES=fused answers the lidar-point and occupancy queries with one `HotPath.point_queries` call (default:
# split, one `sample_points` call per sample and volume plus `occupancy_queries`), VAMP_CONV3D_EPILOGUE=1 fuses what
# follows a 3-D convolution (bias, residual add, LeakyReLU, the heads' slices and sigmoid) into the convolution kernel's
# store (default: the torch expressions).
# Tests and tools flip the attributes of `SWITCHES`.
class _Switches:
    conv3d = os.environ.get("VAMP_CONV3D", "1") != "0"
    conv3d_min_voxels = int(os.environ.get("VAMP_CONV3D_MIN_VOXELS", "50000"))
    # the stride-2 layers (Hourglass3D.conv1 / conv3) under a 16-bit autocast; needs `conv3d` on as well.  Default on:
    # forward + backward 94 / 79 us against MIOpen's 169 / 113 us at the two cfg-B layers (profiles/conv_s2_16bit.txt)
    conv3d_s2 = os.environ.get("VAMP_CONV3D_S2", "1") != "0"
    hip_glue = os.environ.get("VAMP_GLUE", "aten") == "hip"
    # SURVEY 8f N2, the fused forms (default on): the depth softmax runs inside the lift's operand launch
    # and its backward inside the lift backward's gather; VAMP_FUSE=0 restores softmax -> lift
    fuse = os.environ.get("VAMP_FUSE", "1") != "0"
    # the 2-D bilinear resizes between render and losses (bv2:616-626, 203-209) on the HIP kernels: one launch for the
    # three camera maps, a gather backward without float atomics.  Replayed from a graph forward + backward takes
    # 63 us against aten's 262 us for the maps and 43 against 81 us for cfg-A's BEV feature (batch 1,
    # profiles/resize2d.json); default off all the same: eager the path is host-bound and lost on the BEV feature in
    # one of five runs
    resize2d = os.environ.get("VAMP_RESIZE2D", "0") == "1"
    # the point queries of bv2:576-609: "split" = 2 B + 2 `sample_points` calls, each an autograd node with a cell list
    # and a full-size gradient volume of its own; "fused" = one `point_queries` call, one backward
    queries = os.environ.get("VAMP_QUERIES", "split")
    # y = act(conv(x, w) + bias + residual) as one operator and one autograd node (`layers.conv3d_fused`,
    # `layers.conv3d_heads`) wherever `conv3d_kind` names a HIP kernel for the layer: twelve of the UNet's
    # thirteen convolutions, the three heads, and the layers with a bias.  Default off until profiles/conv_epilogue.json
    # argues otherwise.
    conv3d_epilogue = os.environ.get("VAMP_CONV3D_EPILOGUE", "0") == "1"


SWITCHES = _Switches()


def _resize2d_pack(tensors, size):
    """The HIP resize of `tensors` ([..., H, W], one launch) when `SWITCHES.resize2d` is on, they are fp32 device
    tensors and the kernels take the ratio; None otherwise: the caller keeps its aten path."""
    if not (SWITCHES.resize2d and all(t.is_cuda and t.dtype == torch.float32 and t.numel() for t in tensors)):
        return None
    from .layers import resize_bilinear2d_pack, resize_bilinear2d_supported
    if not resize_bilinear2d_supported(tensors[0].shape[-2:], size):
        return None
    return resize_bilinear2d_pack(tensors, size)


def _switched_kind(x, weight, stride, padding, has_bias):
    """The kind `layers.conv3d_kind` names for the layer under `SWITCHES` and the current autocast, or None."""
    if not SWITCHES.conv3d:
        return None
    return conv3d_kind(x.shape, weight.shape, x.dtype, weight.dtype, x.is_cuda, stride, padding, has_bias,
                       autocast=cuda_autocast(), min_voxels=SWITCHES.conv3d_min_voxels, stride2=SWITCHES.conv3d_s2)


def _hip_conv3d(x, weight, stride, padding, bias):
    """The layer on the HIP kernels `layers.conv3d_kind` names for it under `SWITCHES` and the current autocast (the
    reference's mixed-precision training: 16-bit operands, as autocast would hand them to MIOpen), or None: the caller
    keeps aten / MIOpen."""
    kind = _switched_kind(x, weight, stride, padding, bias is not None)
    if kind is None:
        return None
    if kind == "fp32":
        return conv3d_3x3x3(x, weight)
    dt16 = cuda_autocast()
    return (conv3d_bf16 if kind == "half" else conv3d_bf16_stride2)(x.to(dt16), weight.to(dt16))


def _layer_kind(x, weight, stride, padding):
    """The kind of HIP convolution the epilogue operators would run the layer on under `SWITCHES` and the current
    autocast (a bias is theirs to add), or None."""
    return _switched_kind(x, weight, stride, padding, False) if SWITCHES.conv3d_epilogue else None


def _fused_conv3(layer, x, residual=None, act=None, slope=0.01):
    """act(layer(x) + residual) as one `conv3d_fused` call (the layer's bias included), or None where no HIP kernel
    takes the layer."""
    if _layer_kind(x, layer.weight, layer.stride, layer.padding) is None:
        return None
    return conv3d_fused(x, layer.weight, layer.bias, residual, act, slope, layer.stride[0])


def _conv3_then(layer, x, residual=None, leaky=False):
    """leaky_relu(layer(x) + residual), the add and the activation as asked: fused into the convolution where a HIP
    kernel takes the layer, today's torch expressions where none does."""
    y = _fused_conv3(layer, x, residual, "leaky_relu" if leaky else None)
    if y is not None:
        return y
    y = layer(x)
    if residual is not None:
        y = y + residual
    return F.leaky_relu(y, inplace=True) if leaky else y


class _Conv3(nn.Conv3d):
    """nn.Conv3d(cin, cout, 3, stride, 1, bias=False) (same parameter name and shape).  The
    stride-1 layers with 16 / 32 channels run on the HIP fp32 matrix-core kernels for fp32 device
    tensors of at least `VAMP_CONV3D_MIN_VOXELS` voxels (default 50 000: 1.7x MIOpen forward +
    backward at 16x200x200, 1.1x at 8x100x100; the coarsest level is latency-bound and stays with
    MIOpen); `VAMP_CONV3D=0` keeps MIOpen everywhere.  Under a 16-bit autocast the stride-1 layers run on
    conv3d_bf16.hip and the stride-2 ones on conv3d_bf16_s2.hip (`VAMP_CONV3D_S2=0`: MIOpen).  A layer built with a
    bias reaches the HIP kernels only through their bias epilogue (`VAMP_CONV3D_EPILOGUE=1`)."""

    def forward(self, x):
        if self.bias is not None:
            y = _fused_conv3(self, x)
        else:
            y = _hip_conv3d(x, self.weight, self.stride, self.padding, self.bias)
        return super().forward(x) if y is None else y


def _conv3(cin, cout, stride=1):
    return _Conv3(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


class Hourglass3D(nn.Module):
    """Two-level 3-D hourglass with optional skip inputs (layer names follow bv2:32-78)."""

    def __init__(self, mid_channels):
        super().__init__()
        m = mid_channels
        self.conv1 = nn.Sequential(_conv3(m, 2 * m, 2), nn.LeakyReLU(inplace=True))
        self.conv2 = nn.Sequential(_conv3(2 * m, 2 * m))
        self.conv3 = nn.Sequential(_conv3(2 * m, 2 * m, 2), nn.LeakyReLU(inplace=True))
        self.conv4 = nn.Sequential(_conv3(2 * m, 2 * m), nn.LeakyReLU(inplace=True))
        self.conv5 = nn.Sequential(_conv3(2 * m, 2 * m))
        self.conv6 = nn.Sequential(_conv3(2 * m, m))

    def forward(self, x, presqu=None, postsqu=None, skip=None):
        """`skip`: a tensor added to the block's output (Unet3D's residual to the stem), or None.  Every add and
        LeakyReLU goes through `_conv3_then`: inside the convolution before it under `SWITCHES.conv3d_epilogue`, else
        (and on layers no HIP kernel takes) the torch expressions, slope 0.01 like the `nn.LeakyReLU` members."""
        down = _conv3_then(self.conv1[0], x, leaky=True)
        pre = _conv3_then(self.conv2[0], down, postsqu, leaky=True)
        bottom = _conv3_then(self.conv4[0], _conv3_then(self.conv3[0], pre, leaky=True), leaky=True)
        up = _resize(bottom, pre.shape[-3:])
        post = _conv3_then(self.conv5[0], up, pre if presqu is None else presqu, leaky=True)
        out = _resize(post, x.shape[-3:])
        return _conv3_then(self.conv6[0], out, skip), pre, post


class Unet3D(nn.Module):
    """Stem conv + two stacked hourglasses with residuals to the stem (bv2:17-30)."""

    def __init__(self, in_channels, mid_channels):
        super().__init__()
        self.init_dres = _conv3(in_channels, mid_channels)
        self.hg1 = Hourglass3D(mid_channels)
        self.hg2 = Hourglass3D(mid_channels)

    def forward(self, x):
        stem = self.init_dres(x)
        out1, pre1, post1 = self.hg1(stem, skip=stem)      # the two adds of the stem: conv6's residual
        return self.hg2(out1, pre1, post1, skip=stem)[0]


class _StandInEncoder(nn.Module):
    """Used only when mmdet/mmdet3d are absent: strided convs to 1/downsample resolution with
    sum(img_neck_conf['out_channels']) output channels.  NOT the reference's ResNet-50 +
    SECONDFPN -- a placeholder so that the module runs end to end."""

    def __init__(self, out_channels, downsample):
        super().__init__()
        layers, c, s = [], 3, 1
        while s < downsample:
            layers += [nn.Conv2d(c, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True)]
            c, s = 32, s * 2
        layers += [nn.Conv2d(c, out_channels, 3, 1, 1, bias=False), nn.BatchNorm2d(out_channels),
                   nn.ReLU(inplace=True)]
        self.net = nn.Sequential(*layers)

    def init_weights(self):
        pass

    def forward(self, x):
        return self.net(x)


class _Identity(nn.Module):
    def init_weights(self):
        pass

    def forward(self, x):
        return [x] if not isinstance(x, (list, tuple)) else x


def _build_image_encoder(img_backbone_conf, img_neck_conf, downsample):
    try:                                               # the reference's builders (bv2:5-6,167-168)
        from mmdet.models import build_backbone
        from mmdet3d.models import build_neck
        return build_backbone(img_backbone_conf), build_neck(img_neck_conf)
    except ImportError:
        if (img_backbone_conf.get("type") == "ResNet" and img_neck_conf.get("type") == "SECONDFPN"
                and "depth" in img_backbone_conf and "upsample_strides" in img_neck_conf):
            # mmdet / mmdet3d absent: this build's own ResNet + SECOND FPN (vampire_amd/encoders.py)
            from .encoders import build_backbone, build_neck
            return build_backbone(img_backbone_conf), build_neck(img_neck_conf)
        return _StandInEncoder(sum(img_neck_conf["out_channels"]), downsample), _Identity()


# ---------------------------------------------------------------------------
# the backbone
# ---------------------------------------------------------------------------
class BaseVAMPIRE2(nn.Module):
    """The headline backbone (bv2:81).  Its three siblings below differ only in the class-level
    switches `_BASE` (3-D UNet or one Conv3d + Softplus), `_USE_DEPTH` (depth-distribution lift or
    the D = 1 bilinear lift), `_ROTATE_OCC` (occupancy grid rotated by bda or the static
    normalised grid) and in their keyword defaults."""
    _BASE = "unet"
    _USE_DEPTH = True
    _ROTATE_OCC = True

    def __init__(self, x_bound_seg, y_bound_seg, z_bound_seg, x_bound_det, y_bound_det,
                 z_bound_det, d_bound, final_dim, downsample_factor, upsample_factor,
                 mid_channels, output_channels, img_backbone_conf, img_neck_conf, num_classes,
                 density_mode="naive", sdf_bias=-1.0, cat_pos=False, cat_seg=False, use_da=False):
        super().__init__()
        self.downsample_factor = downsample_factor
        self.upsample_factor = upsample_factor
        self.num_classes = num_classes
        self.x_bound_seg, self.y_bound_seg, self.z_bound_seg = x_bound_seg, y_bound_seg, z_bound_seg
        self.x_bound_det, self.y_bound_det, self.z_bound_det = x_bound_det, y_bound_det, z_bound_det
        self.d_bound = d_bound
        self.final_dim = final_dim
        self.mid_channels = mid_channels
        self.output_channels = output_channels
        self.density_mode = density_mode
        self.sdf_bias = sdf_bias
        self.cat_pos = cat_pos
        self.cat_seg = cat_seg
        self.use_da = use_da
        self.path_cfg = PathConfig(
            x_bound_seg=tuple(x_bound_seg), y_bound_seg=tuple(y_bound_seg), z_bound_seg=tuple(z_bound_seg),
            x_bound_det=tuple(x_bound_det), y_bound_det=tuple(y_bound_det), z_bound_det=tuple(z_bound_det),
            d_bound=tuple(d_bound), final_dim=tuple(final_dim), downsample_factor=downsample_factor,
            mid_channels=mid_channels, num_classes=num_classes,
            density_mode="sdf" if density_mode == "sdf" else "naive", sdf_bias=sdf_bias, cat_seg=cat_seg)

        # buffers: names / shapes / values as in the reference (checkpoint compatibility)
        self.register_buffer("frustum", G.make_frustum(final_dim, downsample_factor, d_bound))
        self.fD = self.frustum.shape[0] - 1
        self.fH, self.fW = self.frustum.shape[1], self.frustum.shape[2]
        self.register_buffer("camera_mids", G.make_camera_mids(d_bound))
        self.register_buffer("bev_mids", G.make_bev_mids(z_bound_det))
        self.register_buffer("voxel_coords", G.make_voxel_coords(x_bound_seg, y_bound_seg, z_bound_seg))
        occ = G.make_occ_coords()
        if self._ROTATE_OCC:
            self.register_buffer("occ_coords", occ)                  # bv2:148
        else:
            # base_lss_impaintor.py:152, 297-314 (same in base_lss.py / base_bilinear.py): the grid
            # normalised by the seg bounds once, at construction
            lo = torch.as_tensor([x_bound_seg[0], y_bound_seg[0], z_bound_seg[0]])
            span = torch.as_tensor([x_bound_seg[1] - x_bound_seg[0], y_bound_seg[1] - y_bound_seg[0],
                                    z_bound_seg[1] - z_bound_seg[0]])
            self.register_buffer("norm_occ_coords", ((occ - lo) / span) * 2.0 - 1.0)
            # the raw grid for the kernels (they normalise themselves): a non-persistent buffer, so that it
            # follows module.to() / .cuda() and the state-dict keys stay the reference's
            self.register_buffer("_occ_points", occ, persistent=False)
        if cat_pos:
            self.register_buffer("norm_voxel_coords",
                                 G.make_voxel_coords(x_bound_seg, y_bound_seg, z_bound_seg, norm=True))
        self.register_buffer("output_coords", G.make_voxel_coords(x_bound_det, y_bound_det, z_bound_det))
        self.vZ, self.vY, self.vX = self.voxel_coords.shape[:3]
        self.oY = self.output_coords.shape[1]
        self.depth_channels = self.frustum.shape[0]

        self.img_backbone, self.img_neck = _build_image_encoder(img_backbone_conf, img_neck_conf,
                                                                downsample_factor)
        img_out = sum(img_neck_conf["out_channels"])
        if self._USE_DEPTH:
            self.mapping_along_depth = nn.Sequential(nn.Conv2d(img_out, self.depth_channels, 3, 1, 1, bias=False))
        self.channel_lower = nn.Conv2d(img_out, mid_channels, 3, 1, 1, bias=False)
        vin = mid_channels + (3 if cat_pos else 0)
        if self._BASE == "unet":
            self.base_conv = Unet3D(vin, mid_channels)
        else:                                                        # base_lss.py:117-124, base_bilinear.py:173-179
            self.base_conv = nn.Sequential(_Conv3(vin, mid_channels, 3, 1, 1, bias=True), nn.Softplus(beta=100))
        self.density_conv = nn.Conv3d(mid_channels, 1, 3, 1, 1, bias=True)
        self.seg_conv = nn.Conv3d(mid_channels, num_classes, 3, 1, 1, bias=True)
        if not self._USE_DEPTH:
            self.feature_conv = _Conv3(mid_channels, mid_channels, 3, 1, 1, bias=True)      # base_bilinear.py:182
        self.density = nn.Sigmoid() if density_mode == "naive" else \
            ModifyLaplaceDensity(beta=0.1, bias=sdf_bias)
        self.rgb_conv = nn.Sequential(nn.Conv3d(mid_channels, 3, 3, 1, 1, bias=True), nn.Sigmoid())
        vo_in = (mid_channels + (num_classes if cat_seg else 0)) * self.output_coords.shape[0]
        # The reference defines voxel_output only for a 128- or 256-cell BEV side (bv2:203-209);
        # other sides (e.g. the 200x200 grid of BASELINE.json) get the plain 1x1 conv (superset).
        if self.oY == 256:
            self.voxel_output = nn.Sequential(nn.Conv2d(vo_in, output_channels, 1, 1, bias=True),
                                              nn.UpsamplingBilinear2d(scale_factor=0.5))
        else:
            self.voxel_output = nn.Conv2d(vo_in, output_channels, 1, 1, bias=True)
        self.upsample2d = nn.UpsamplingBilinear2d(scale_factor=upsample_factor)
        self.init_weights()
        self.img_neck.init_weights()
        self.img_backbone.init_weights()
        self._hot = None

    # -- weights ------------------------------------------------------------
    def init_weights(self):
        """He-style normal init of the conv layers, density bias pushed far below the sdf
        bias (bv2:216-241)."""
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                fan = m.out_channels * math.prod(m.kernel_size)
                m.weight.data.normal_(0, math.sqrt(2.0 / fan))
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.bias.data.zero_()
                nn.init.normal_(m.weight, 0.0, math.sqrt(2) / math.sqrt(m.weight.shape[1]))
        nn.init.constant_(self.density_conv.bias, self.sdf_bias - 10.0)

    # -- hot path handle ----------------------------------------------------
    def hot_path(self) -> HotPath:
        dev = self.frustum.device
        if self._hot is None or self._hot.device != dev:
            self._hot = HotPath(self.path_cfg, dev)
        return self._hot

    def _beta(self):
        return self.density.beta if self.density_mode == "sdf" else None

    # -- geometry (bv2:314-388) ---------------------------------------------
    def get_geometry(self, sensor2ego_mat, intrin_mat, ida_mat, bda_mat):
        """Frustum points in the ego frame, [B, N, D, fH, fW, 3] (HIP kernel)."""
        mats = G.render_matrices(sensor2ego_mat, intrin_mat, ida_mat, bda_mat)
        return self.hot_path().frustum_geometry(mats)

    def get_pixel(self, sensor2ego_mat, intrin_mat, ida_mat, bda_mat):
        """Voxel centres in (u, v, depth), [B, N, vZ, vY, vX, 3].  Only needed by callers that
        want the coordinates themselves (the lift projects in-kernel); small torch ops."""
        B, N = sensor2ego_mat.shape[:2]
        m = G.lift_matrices(sensor2ego_mat, intrin_mat, ida_mat, bda_mat).view(B, N, 3, 1, 1, 1, 4, 4)
        p = m[:, :, 0].matmul(self.voxel_coords.unsqueeze(-1))
        p = m[:, :, 1].matmul(p)
        z = torch.clamp(p[..., 2:3, :], min=1e-6)
        p = torch.cat((p[..., :2, :] / z, p[..., 2:, :]), dim=-2)
        return m[:, :, 2].matmul(p).squeeze(-1)[..., :3]

    # -- LIFT (bv2:483-516) -------------------------------------------------
    def get_voxel_feats(self, frustum_feats, sweep_index, mats_dict, clamp_extreme=True):
        """Signature-compatible lift from the materialised [B, N, C, D, fH, fW] tensor.

        `clamp_extreme` (bv2:503-505) is accepted with either value and changes nothing: the clamp
        to [-2, 2] only moves normalised coordinates of samples that `valid` (bv2:494-497, computed
        before it) has already masked to zero -- a valid sample has |n| <= 1 + 1/703 -- and the
        kernel evaluates valid samples only."""
        mats = G.lift_matrices(mats_dict["sensor2ego_mats"][:, sweep_index],
                               mats_dict["intrin_mats"][:, sweep_index],
                               mats_dict["ida_mats"][:, sweep_index], mats_dict.get("bda_mat", None))
        if not self._USE_DEPTH:
            # base_bilinear.py:471-519: img_feats [B, N, C, fH, fW], 2-D bilinear sample, z_valid = z > 0
            return self.hot_path().lift(None, frustum_feats.float(), mats, use_depth=False)
        return self.hot_path().lift_dense(frustum_feats.float(), mats)

    def _lift_mats(self, sweep_index, mats_dict):
        return G.lift_matrices(mats_dict["sensor2ego_mats"][:, sweep_index],
                               mats_dict["intrin_mats"][:, sweep_index],
                               mats_dict["ida_mats"][:, sweep_index], mats_dict.get("bda_mat", None))

    def lift(self, depth, feat, sweep_index, mats_dict):
        """Fused lift: depth [B,N,D,fH,fW] and feat [B,N,C,fH,fW]; no outer product."""
        return self.hot_path().lift(depth, feat, self._lift_mats(sweep_index, mats_dict))

    # -- RENDER (bv2:391-467) -----------------------------------------------
    def volume_rendering_from_multiple_views(self, geom_xyz, density_feature, semantic_logits,
                                             voxel_features, rgb):
        return self.hot_path().render(density_feature.float(), semantic_logits.float(),
                                      voxel_features.float(), rgb.float(), self._beta(), geom=geom_xyz)

    def render(self, mats_dict, sweep_index, density_feature, semantic_logits, voxel_features, rgb):
        """Renderer with in-kernel frustum geometry (get_geometry + nan_to_num fused)."""
        mats = G.render_matrices(mats_dict["sensor2ego_mats"][:, sweep_index],
                                 mats_dict["intrin_mats"][:, sweep_index],
                                 mats_dict["ida_mats"][:, sweep_index], mats_dict.get("bda_mat", None))
        return self.hot_path().render(density_feature.float(), semantic_logits.float(),
                                      voxel_features.float(), rgb.float(), self._beta(),
                                      render_mats=mats)

    # -- image features (bv2:469-481) ---------------------------------------
    def get_cam_feats(self, imgs):
        B, S, N, C, H, W = imgs.shape
        feats = self.img_neck(self.img_backbone(imgs.reshape(B * S * N, C, H, W)))[0]
        return feats.reshape(B, S, N, feats.shape[1], feats.shape[2], feats.shape[3])

    def _norm_by_seg_bounds(self, pts):
        lo = pts.new_tensor([self.x_bound_seg[0], self.y_bound_seg[0], self.z_bound_seg[0]])
        span = pts.new_tensor([self.x_bound_seg[1] - self.x_bound_seg[0],
                               self.y_bound_seg[1] - self.y_bound_seg[0],
                               self.z_bound_seg[1] - self.z_bound_seg[0]])
        return (pts - lo) / span * 2.0 - 1.0

    # -- one sweep (bv2:518-649) --------------------------------------------
    def _heads(self, base):
        """density_conv / seg_conv / rgb_conv (bv2:186-198): three 3x3x3 convs of the same input.  For
        fp32 device tensors they run as ONE 16 -> 32 HIP conv on the concatenated (zero-padded)
        weights -- the volume is read once and MIOpen's three forward / data / weight-gradient
        launches become one each; biases and the rgb sigmoid follow.  Parameters are untouched."""
        nout = 1 + self.num_classes + 3
        if SWITCHES.conv3d and nout <= 32 and base.dim() == 5 and base.is_cuda:
            wd, ws, wr = self.density_conv.weight, self.seg_conv.weight, self.rgb_conv[0].weight
            w = torch.cat([wd, ws, wr, wd.new_zeros((32 - nout,) + tuple(wd.shape[1:]))], 0)
            if _layer_kind(base, w, (1, 1, 1), (1, 1, 1)) is not None:
                # the three slices, bias adds and the sigmoid in the convolution's store: no padded y, fp32 outputs
                f32 = torch.float32
                return conv3d_heads(base, w, [HeadSegment(1, self.density_conv.bias, None, f32),
                                              HeadSegment(self.num_classes, self.seg_conv.bias, None, f32),
                                              HeadSegment(3, self.rgb_conv[0].bias, "sigmoid", f32)])
            y = _hip_conv3d(base, w, (1, 1, 1), (1, 1, 1), None)
            if y is not None:
                K = self.num_classes
                bias = lambda b: b.view(1, -1, 1, 1, 1)
                return (y[:, :1] + bias(self.density_conv.bias), y[:, 1:1 + K] + bias(self.seg_conv.bias),
                        torch.sigmoid(y[:, 1 + K:nout] + bias(self.rgb_conv[0].bias)))
        return self.density_conv(base), self.seg_conv(base), self.rgb_conv(base)

    def _forward_single_sweep(self, sweep_index, sweep_imgs, mats_dict, inrange_pts=None):
        return self._sweep_from_feats(sweep_index, self.get_cam_feats(sweep_imgs), mats_dict, inrange_pts)

    def _sweep_from_feats(self, sweep_index, img_feats, mats_dict, inrange_pts=None, occupancy=True):
        """bv2:548-649 from the neck features [B, S, N, c, fH, fW] on (everything behind get_cam_feats);
        `occupancy=False` leaves the Occ3D resampling out (the last two outputs are None): the
        data-parallel harness of step.py uses it on CPU, where the oracle stands in for the kernels."""
        B, S, N = img_feats.shape[:3]
        src = img_feats[:, 0].reshape(B * N, -1, img_feats.shape[-2], img_feats.shape[-1])
        hp = self.hot_path()
        feat = self.channel_lower(src).reshape(B, N, -1, *src.shape[-2:])
        # the HIP depth-softmax / density-gate kernels are 3-5x faster than aten's as
        # kernels, but at batch 1 their host glue (ctypes call, autograd.Function, layout fix-ups)
        # costs what they save (156 vs 149 us and 167 vs 104 us end to end, profiles/widening_rows_r01f.txt),
        # so the module runs the reference's aten expressions unless VAMP_GLUE=hip asks for the kernels
        # (they stay available and tested: HotPath.depth_softmax / density_gate).
        hip_glue = SWITCHES.hip_glue
        if self._USE_DEPTH:
            logits = self.mapping_along_depth(src)
            if SWITCHES.fuse and hasattr(hp, "lift_logits"):
                # bv2:550 + 553 fused: the lift takes the logits (softmax in its operand launch, softmax
                # backward in its gather); no depth tensor in the autograd graph
                voxel_features = hp.lift_logits(logits.reshape(B, N, -1, *src.shape[-2:]), feat.float(),
                                                self._lift_mats(sweep_index, mats_dict))
            else:
                depth = hp.depth_softmax(logits) if hip_glue else logits.float().softmax(dim=1)   # bv2:550
                depth = depth.reshape(B, N, -1, *src.shape[-2:])
                voxel_features = self.lift(depth, feat.float(), sweep_index, mats_dict)
        else:
            voxel_features = self.get_voxel_feats(feat, sweep_index, mats_dict)     # base_bilinear.py:566
        if self.cat_pos:
            pos = self.norm_voxel_coords.permute(3, 0, 1, 2)[None].repeat(B, 1, 1, 1, 1)
            voxel_features = torch.cat([voxel_features, pos], dim=1)
        base = self.base_conv(voxel_features)
        if self._USE_DEPTH:
            density_feature, semantic_logits, rgb = self._heads(base)
        else:
            # base_bilinear.py:575-578: rgb and the rendered features come from feature_conv(base)
            density_feature, semantic_logits = self.density_conv(base), self.seg_conv(base)
            base = self.feature_conv(base)
            rgb = self.rgb_conv(base)

        # lidar-point queries (bv2:576-596) and occupancy resampling on the bda-rotated Occ3D grid
        # (bv2:597-609): HIP point resampling, `hp` may be an oracle stand-in on CPU
        beta = self._beta()
        if SWITCHES.queries == "fused" and hasattr(hp, "point_queries"):
            pts_logits_batch, pts_sdf_batch, occ_logits, occ_density = self._fused_queries(
                hp, semantic_logits, density_feature, beta, mats_dict, inrange_pts, occupancy)
        else:
            pts_logits_batch, pts_sdf_batch = [], []
            if inrange_pts is not None:
                for i in range(B):
                    pts = inrange_pts[i][None].float()
                    pts_logits_batch.append(hp.sample_points(semantic_logits[[i]].float(), pts, padding="border",
                                                             channel_last=True)[0])
                    if self.density_mode == "sdf":
                        pts_sdf_batch.append(hp.sample_points(density_feature[[i]].float(), pts,
                                                              mask_outside=True)[0, 0])
            if not occupancy:
                occ_logits = occ_density = None
            elif self._ROTATE_OCC:
                occ_logits, occ_density = hp.occupancy_queries(semantic_logits.float(), density_feature.float(),
                                                               self.occ_coords, mats_dict.get("bda_mat", None), beta)
            else:
                # static grid (base_lss_impaintor.py:611-616): the same queries without the bda rotation
                occ_logits, occ_density = hp.occupancy_queries(semantic_logits.float(), density_feature.float(),
                                                               self._occ_points, None, beta)

        (rgb_p, seg_p, depth_p, bev_rgb, bev_seg, bev_height, bev_density, voxel_output) = \
            self.render(mats_dict, sweep_index, density_feature, semantic_logits, base, rgb)

        maps = [t.reshape(B, N, -1, self.fH, self.fW) for t in (rgb_p, seg_p, depth_p)]
        up_size = (math.floor(self.fH * self.upsample_factor), math.floor(self.fW * self.upsample_factor))
        resized = _resize2d_pack(maps, up_size)                    # bv2:616-626 in one launch (SWITCHES.resize2d)
        if resized is not None:
            rgb_p, seg_p, depth_p = resized
        else:
            up = lambda t: self.upsample2d(t.reshape(B * N, -1, self.fH, self.fW)).reshape(
                B, N, -1, self.fH * self.upsample_factor, self.fW * self.upsample_factor)
            rgb_p, seg_p, depth_p = up(rgb_p), up(seg_p), up(depth_p)
        conv = self.voxel_output[0] if isinstance(self.voxel_output, nn.Sequential) else self.voxel_output
        if (SWITCHES.fuse and hasattr(hp, "gate_conv1x1")
                and hp.gate_conv1x1_supported(voxel_output.shape[1], voxel_output.shape[2], conv.out_channels)):
            # bv2:627-632 fused: gate and 1x1 conv in one matrix-core kernel, the gated tensor never exists
            bev_feat = hp.gate_conv1x1(voxel_output, bev_density, conv.weight, conv.bias)
            if conv is not self.voxel_output:
                bev_feat = self._half_resize(bev_feat)             # the 256-cell grid's 0.5x bilinear resize (bv2:205)
        else:
            if hip_glue:
                voxel_output = hp.density_gate(voxel_output, bev_density)  # bv2:627-630, HIP consumer kernel
            else:
                voxel_output = voxel_output * (bev_density.tanh() if self.density_mode == "sdf" else bev_density)
            bev_feat = conv(voxel_output.reshape(B, -1, *voxel_output.shape[-2:]))
            if conv is not self.voxel_output:
                bev_feat = self._half_resize(bev_feat)
            bev_feat = bev_feat.float()
        return (bev_feat.contiguous(), rgb_p, seg_p, depth_p, bev_rgb, bev_seg, bev_height,
                bev_density, pts_logits_batch, pts_sdf_batch,
                None if occ_logits is None else occ_logits.permute(0, 2, 3, 4, 1),
                None if occ_density is None else occ_density.permute(0, 2, 3, 4, 1).tanh())

    def _fused_queries(self, hp, semantic_logits, density_feature, beta, mats_dict, inrange_pts, occupancy):
        """The queries of bv2:576-609 as ONE `point_queries` call (SWITCHES.queries == "fused"): (pts_logits_batch,
        pts_sdf_batch, occ_logits, occ_density) with the shapes of the split path -- the per-sample results are the
        slices [b, :n_b] of the packed outputs."""
        B = semantic_logits.shape[0]
        sdf = self.density_mode == "sdf"
        points = None if inrange_pts is None else [inrange_pts[i].float() for i in range(B)]
        occ_points = shp = None
        if occupancy:
            if self._ROTATE_OCC:
                grid, bda = self.occ_coords, mats_dict.get("bda_mat", None)
            else:       # static grid (base_lss_impaintor.py:611-616): [1, P, 3] for all samples
                grid, bda = self._occ_points, None
            occ_points, shp = hp.occupancy_points(grid, bda), tuple(grid.shape[:3])
        pts_logits_batch, pts_sdf_batch, occ_logits, occ_density = [], [], None, None
        if points is None and occ_points is None:
            return pts_logits_batch, pts_sdf_batch, occ_logits, occ_density
        q = hp.point_queries(semantic_logits.float(), density_feature.float(), beta, points=points,
                             sdf=sdf and points is not None, occ_points=occ_points, lattice=shp)
        if points is not None:
            pts_logits_batch = [q.pts_logits[b, :p.shape[0]] for b, p in enumerate(points)]
            if sdf:
                pts_sdf_batch = [q.pts_sdf[b, :p.shape[0]] for b, p in enumerate(points)]
        if occ_points is not None:
            occ_logits, occ_density = q.occ_logits.reshape(B, -1, *shp), q.occ_density.reshape(B, 1, *shp)
        return pts_logits_batch, pts_sdf_batch, occ_logits, occ_density

    def _half_resize(self, x):
        """`voxel_output[1]`, the 0.5x UpsamplingBilinear2d of the 256-cell grid (bv2:205): resize2d.hip when
        `SWITCHES.resize2d` admits the tensor, else the module itself."""
        resized = _resize2d_pack([x], tuple(math.floor(v * 0.5) for v in x.shape[-2:]))
        return self.voxel_output[1](x) if resized is None else resized[0]

    def forward(self, sweep_imgs, mats_dict, inrange_pts=None, timestamps=None):
        if sweep_imgs.shape[1] != 1:
            raise NotImplementedError          # as the reference (bv2:690-693)
        return self._forward_single_sweep(0, sweep_imgs[:, 0:1], mats_dict, inrange_pts=inrange_pts)


class BaseLSSImpaintor(BaseVAMPIRE2):
    """src/layers/backbones/base_lss_impaintor.py:79: BaseVAMPIRE2 with the static `norm_occ_coords`
    buffer (the occupancy grid is not rotated by bda, :611-616) and cat_pos / cat_seg on by default
    (:100-101)."""
    _ROTATE_OCC = False

    def __init__(self, x_bound_seg, y_bound_seg, z_bound_seg, x_bound_det, y_bound_det, z_bound_det, d_bound,
                 final_dim, downsample_factor, upsample_factor, mid_channels, output_channels,
                 img_backbone_conf, img_neck_conf, num_classes, density_mode="naive", sdf_bias=-1.0,
                 cat_pos=True, cat_seg=True, use_da=False):
        super().__init__(x_bound_seg, y_bound_seg, z_bound_seg, x_bound_det, y_bound_det, z_bound_det, d_bound,
                         final_dim, downsample_factor, upsample_factor, mid_channels, output_channels,
                         img_backbone_conf, img_neck_conf, num_classes, density_mode, sdf_bias, cat_pos,
                         cat_seg, use_da)


class BaseLSS(BaseLSSImpaintor):
    """src/layers/backbones/base_lss.py:16: the ablation whose `base_conv` is one Conv3d + Softplus
    (:117-124) instead of the 3-D UNet."""
    _BASE = "conv"


class BaseBiLinear(BaseVAMPIRE2):
    """src/layers/backbones/base_bilinear.py:80: no depth distribution -- `get_voxel_feats(img_feats,
    ...)` is a 2-D bilinear sample of [B, N, C, fH, fW] with z_valid = z > 0 (:471-519; the HIP lift
    with use_depth = 0), `base_conv` = Conv3d + Softplus, an extra `feature_conv` feeds rgb and the
    renderer (:575-578), static `norm_occ_coords`."""
    _BASE = "conv"
    _USE_DEPTH = False
    _ROTATE_OCC = False
