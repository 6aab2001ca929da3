"""Build switches of the MI355X path as ONE frozen object, fixed at model construction.

`import_and_load(..., config=Config(...))` attaches the object to every sub-module of the network it builds
(`attach(model, cfg)`); the networks read `cfg(self).<switch>` and hand operator-level switches to the operator table as
keyword arguments (`CorrBlock(..., bwd_windows=...)`, `pwc_warp(..., deterministic=...)`, `dense_block(..., fused_masks=...)`,
`attention_softmax(..., gemm=..., mfma=...)`).  Nothing flips a module global after import: an A/B run builds a second model (the
weights are seeded, the packs are cached per tensor) with `dataclasses.replace(DEFAULT, switch=value)`.

Every switch selects between two executions of the same arithmetic (parity-tested against each other); the defaults are
the product path.  Environment variables only set the DEFAULT object, once, at import."""
import dataclasses
import os


def _env_bool(name, default):
    v = os.environ.get(name)
    return default if v is None else v not in ("0", "", "false", "False")


@dataclasses.dataclass(frozen=True)
class Config:
    # ---- RAFT / GMA (nets/raft.py, nets/gma.py) ----
    fused_lookup: bool = True            # lookup -> convc1 -> bias -> ReLU in one launch (ops.corr._CorrLookupConv)
    overlap_encoders: bool = False       # context encoder on a second stream beside the feature encoder (opt-in)
    conv_s2: bool = True                 # stride-2 layers on ops.conv_s2 (False: library convolution)
    conv_s2_bwd: bool = True             # their data gradient on pcfa_conv_s2_bwd (False: library gradient)
    fused_downsample: bool = True        # conv1 + downsample[0] of a stride-2 residual block in one launch
    defer_relu: bool = True              # ReLU backward of single-consumer layers inside neighbouring kernels
    pyramid_bwd_windows: bool = True     # pyramid backward over the lookup windows only (False: dense products)
    gma_gemm: str = "lib"                # GMA attention products: "lib" (rocBLAS through torch.matmul) | "hip" (pcfa_gemm_f32)
    gma_attention: str = "materialised"  # GMA attention: "materialised" ([N, N] softmax matrix, products per gma_gemm) | "streamed"
                                         # (ops.streamed_attention: tiles recomputed per pass, O(N*d) memory, no library product)
    conv1x1: str = "lib"                 # the encoders' output layer and the mask head's 1x1 layer: "lib" | "hip" (pcfa_gemm_f32:
                                         # a RAFT closure then holds no library kernel at all)
    corr: str = "all_pairs"              # correlation: "all_pairs" (CorrBlock: O(Q^2) pyramid, fused lookup -> convc1) |
                                         # "on_demand" (OnDemandCorrBlock: window dot products per lookup, O(Q*D) memory)
    ondemand_lookup: str = "per_query"   # execution of corr="on_demand"'s lookups: "per_query" (one wave per query) | "tiled" (8x8
                                         # query tiles whose windows share a small box run on the fp32 matrix cores, one
                                         # fixed-point scatter per box element; wide tiles keep the per-query kernels)
    motion_bwd: str = "batched"          # backward of RAFT's motion encoder: "batched" (its two 3x3 data gradients once per closure
                                         # over all refinement iterations, ops.motion_steps; frozen weights, one image, fused
                                         # all-pairs lookup -- anything else runs "per_iteration") | "per_iteration" (one pair of
                                         # launches per iteration, interleaved with the GRU backward); bit-identical results
    mfma: str = "f32"                    # arithmetic of the hand-written GEMM core: "f32" (v_mfma_f32_32x32x2_f32) | "bf16x3" (each
                                         # fp32 operand split into three bf16 pieces, six v_mfma_f32_32x32x16_bf16 products: fp32
                                         # accuracy at 16/6 of the fp32 matrix roof).  Takes effect where that core runs: the
                                         # all-pairs pyramid forward (always), the attention products under gma_gemm="hip", the
                                         # 1x1 layers under conv1x1="hip".  Stay fp32: the pyramid backward (sparse-window
                                         # products, pooling adjoint), corr="on_demand", gma_attention="streamed"
    # ---- PWC-Net (nets/pwcnet.py) ----
    dilated_as_subgrids: tuple = (2, 4, 8, 16)   # dilations run as d*d plain 3x3 convolutions on sub-grids (() = library)
    deconv_fewout: bool = True           # deconv / upfeat layers and the x4 up-sampling on own deterministic kernels
    defer_leaky: bool = True             # LeakyReLU backward of single-consumer layers in the consumer's epilogue
    dense_block_fused_masks: bool = True   # the same inside the dense decoder blocks
    warp_bwd_deterministic: bool = True  # fixed-point scatter in the warp backward (False: hardware fp32 atomics)
    pwc_fold_glue: bool = True           # RGB->BGR in conv1a's weights, `up_flow * s` inside the warp, decoder inputs written
                                         # straight into the dense-block buffer, one re-gridding copy between dilated layers
    # ---- SpyNet (nets/spynet.py) ----
    spynet_ops: str = "lib"              # Basic's 7x7 layers, the warp and the flow up-sampling: "lib" (MIOpen, grid_sample,
                                         # interpolate) | "hip" (ops.conv7x7, ops.spynet_warp, ops.upsample_bilinear: no library
                                         # kernel, no atomic-accumulating backward -- reproducible, allowed in flight)
    # ---- FlowNet2 (nets/flownet2.py) ----
    flownet2_ops: str = "lib"            # stride-2 and transposed convolutions, small-map 3x3 layers, conv_redir, Resample2d's
                                         # backward and the x4 up-sampling: "lib" (MIOpen / ATen, fp32 atomics) | "hip"
                                         # (ops.flownet2, ops.conv3x3 at every size: no library kernel, no atomics on float data)
    # ---- attack loop (attack_PCFA.py) ----
    reuse_pair_graphs: bool = True       # pairs of one shape share static buffers + hipGraphs
    max_cached_shapes: int = 4           # graph sets kept per model (LRU); KITTI under /8 padding has three padded shapes

    @classmethod
    def from_env(cls):
        return cls(fused_lookup=_env_bool("PCFA_FUSED_LOOKUP", True),
                   overlap_encoders=_env_bool("PCFA_OVERLAP_ENCODERS", False),
                   defer_relu=_env_bool("PCFA_DEFER_RELU", True),
                   gma_gemm=os.environ.get("PCFA_GMA_GEMM", "lib"),
                   gma_attention=os.environ.get("PCFA_GMA_ATTENTION", "materialised"),
                   conv1x1=os.environ.get("PCFA_CONV1X1", "lib"),
                   corr=os.environ.get("PCFA_CORR", "all_pairs"),
                   ondemand_lookup=os.environ.get("PCFA_ONDEMAND_LOOKUP", "per_query"),
                   motion_bwd=os.environ.get("PCFA_MOTION_BWD", "batched"),
                   mfma=os.environ.get("PCFA_MFMA", "f32"),
                   spynet_ops=os.environ.get("PCFA_SPYNET_OPS", "lib"),
                   flownet2_ops=os.environ.get("PCFA_FLOWNET2_OPS", "lib"),
                   max_cached_shapes=int(os.environ.get("PCFA_MAX_CACHED_SHAPES", "4")))

    def __post_init__(self):
        if self.gma_gemm not in ("lib", "hip"):
            raise ValueError("Config.gma_gemm must be 'lib' or 'hip', got %r" % (self.gma_gemm,))
        if self.gma_attention not in ("materialised", "streamed"):
            raise ValueError("Config.gma_attention must be 'materialised' or 'streamed', got %r" % (self.gma_attention,))
        if self.conv1x1 not in ("lib", "hip"):
            raise ValueError("Config.conv1x1 must be 'lib' or 'hip', got %r" % (self.conv1x1,))
        if self.corr not in ("all_pairs", "on_demand"):
            raise ValueError("Config.corr must be 'all_pairs' or 'on_demand', got %r" % (self.corr,))
        if self.ondemand_lookup not in ("per_query", "tiled"):
            raise ValueError("Config.ondemand_lookup must be 'per_query' or 'tiled', got %r" % (self.ondemand_lookup,))
        if self.motion_bwd not in ("batched", "per_iteration"):
            raise ValueError("Config.motion_bwd must be 'batched' or 'per_iteration', got %r" % (self.motion_bwd,))
        if self.mfma not in ("f32", "bf16x3"):
            raise ValueError("Config.mfma must be 'f32' or 'bf16x3', got %r" % (self.mfma,))
        if self.spynet_ops not in ("lib", "hip"):
            raise ValueError("Config.spynet_ops must be 'lib' or 'hip', got %r" % (self.spynet_ops,))
        if self.flownet2_ops not in ("lib", "hip"):
            raise ValueError("Config.flownet2_ops must be 'lib' or 'hip', got %r" % (self.flownet2_ops,))
        if self.max_cached_shapes < 1:
            raise ValueError("Config.max_cached_shapes must be >= 1")


DEFAULT = Config.from_env()


def attach(model, config=None):
    """Give every sub-module of `model` the (frozen) config; returns the model."""
    config = DEFAULT if config is None else config
    if not isinstance(config, Config):
        raise TypeError("config must be a pcfa_amd.config.Config")
    for m in model.modules():
        object.__setattr__(m, "_pcfa_config", config)   # plain attribute: not a parameter / buffer / sub-module
    return model


def cfg(module):
    """The config a module was built with (DEFAULT for modules constructed on their own, e.g. in unit tests)."""
    return getattr(module, "_pcfa_config", DEFAULT)
