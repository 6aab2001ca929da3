"""The networks' composite modules against float64 autograd: restatements, input builders, kink margins, comparator.

What is compared.  A composite of pcfa_amd/nets (a residual block, an encoder, the update block, the refinement loop, a
PWC-Net chain ...) decides which kernel gets which weight (BatchNorm folded in, [h | rest] / inp slices of the GRU weights,
.25 folded into the mask head, RGB -> BGR folded into conv1a), which tensor carries whose activation mask, which alias
receives a second consumer's gradient and which layout a tensor is in.  Every Case below pairs such an entry (`run`) with
a restatement (`restate`) of the same operation that is written with torch.nn.functional alone from the module's
state_dict, following the behavioural reference's statement (models/raft/extractor.py, update.py, raft.py, corr.py,
utils/utils.py; models/gma/gma.py, update.py, network.py; models/PWCNet/PWCNet.py; models/SpyNet/SpyNet.py;
models/FlowNet/FlowNetS.py, FlowNet2.py, submodules.py and the .cu kernels of Resample2d / ChannelNorm -- the lines the
nets' docstrings cite) and calling nothing of pcfa_amd.nets or pcfa_amd.ops.  The restatement runs in float64 (the reference values) and in float32 (the yardstick of the GPU tier: an
independent fp32 execution of the same operation that shares no code with the product).

Parameters come from a seeded generator with fan-in scaling; every BatchNorm gets non-trivial statistics
(running_mean ~ N(0, .3), running_var ~ U(.5, 2), weight ~ U(.5, 1.5), bias ~ N(0, .3)) and every convolution a
non-zero bias, so that a fold that is the identity on default statistics shows.  Outputs and the gradient with respect to
every differentiable input are compared tensor by tensor.

Kinks.  One ReLU / LeakyReLU unit that an fp32 run and float64 decide differently moves a module gradient by about
1 / sqrt(N), so a tight gate means something only where that cannot happen: the restatement records min|pre| / max|pre| of
every pre-activation tensor and, for the bilinear warps (where the coordinate is differentiated; RAFT's lookups get
detached coordinates), the distance in pixels of every sampling coordinate to the nearest integer (tap changes, borders),
to the clamp and of the validity mask to its threshold.  Entries that are exactly zero in every precision and pass no
gradient on either side -- a residual sum of two ReLU zeros, a cost-volume tap in the zero padding -- are no kinks and are
left out (Tape.relu / Tape.leaky say why).  A case's seed is the first seed >= 0
with every activation margin >= 2^-20 and every coordinate margin >= 2^-10 (`first_clean_seed`, float64 on the CPU, at
most 64 seeds); it is committed as a constant and re-asserted by both tiers before any number of the code under test is
looked at.  A seed is never chosen by what the code under test returns.

No GPU import at module level: the CPU tier imports this file on machines without one.
"""
import collections
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

RELU_MARGIN = 2.0 ** -20
COORD_MARGIN = 2.0 ** -10
MAX_SEEDS = 64


# --------------------------------------------------------------------------- the record of non-smooth quantities
class Tape:
    """What a restatement passes through that is not smooth: pre-activations and sampling coordinates."""

    def __init__(self):
        self.act, self.coord = [], []

    def _pre(self, x, exact_zeros=False):
        a = x.detach().abs()
        top = a.max()
        if exact_zeros:
            a = a[a > 0]
        self.act.append(float(a.min() / top))

    def relu(self, x, sum_of_relus=False):
        """sum_of_relus: x = relu(a) + relu(b), the residual sum inside an encoder.  It is exactly zero where both terms
        are, in every precision as long as a and b keep their own margins (recorded where they were activated), and the
        unit then passes no gradient on either side of the kink: those entries are left out of min|pre|."""
        self._pre(x, sum_of_relus)
        return F.relu(x)

    def leaky(self, x, slope=0.1, zero_padded=False):
        """zero_padded: x is a cost volume, exactly zero where the displaced window lies in the zero padding (or on warped
        features the validity mask zeroed) -- in every precision, and with a zero derivative on both sides of the kink (the
        other factor of the product is the padding): those entries are left out of min|pre|."""
        self._pre(x, zero_padded)
        return F.leaky_relu(x, slope)

    def distance(self, d):
        """d: distances in pixels to the nearest point where the sampled function has a kink."""
        self.coord.append(float(d.detach().min()))

    def clean(self):
        return all(m >= RELU_MARGIN for m in self.act) and all(m >= COORD_MARGIN for m in self.coord)

    def worst(self):
        return min(self.act, default=1.0), min(self.coord, default=1.0)


# --------------------------------------------------------------------------- parameters
def randomise(module, gen):
    """Seeded values for every parameter and BatchNorm statistic of `module`, in place."""
    def randn(shape, std):
        return torch.randn(tuple(shape), generator=gen) * std

    def rand(shape, lo, hi):
        return lo + (hi - lo) * torch.rand(tuple(shape), generator=gen)

    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.ConvTranspose2d):
                fan = m.in_channels * m.kernel_size[0] * m.kernel_size[1] / (m.stride[0] * m.stride[1])
            elif isinstance(m, nn.Conv2d):
                fan = m.weight[0].numel()
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                m.weight.copy_(randn(m.weight.shape, math.sqrt(2.0 / fan)))
                if m.bias is not None:
                    m.bias.copy_(randn(m.bias.shape, 0.1))
            elif isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(randn(m.running_mean.shape, 0.3))
                m.running_var.copy_(rand(m.running_var.shape, 0.5, 2.0))
                m.weight.copy_(rand(m.weight.shape, 0.5, 1.5))
                m.bias.copy_(randn(m.bias.shape, 0.3))
        for name, p in module.named_parameters():
            if name.endswith("gamma"):   # GMA's Aggregate: zero at construction, which would hide the aggregation
                p.copy_(rand(p.shape, 0.5, 1.5))
    return module


def materialise(case, seed):
    """(the module with its seeded fp32 parameters, on the CPU; the case's fp32 inputs)."""
    gen = torch.Generator().manual_seed(seed)
    module = randomise(case.make_module(), gen)
    return module, case.make_inputs(gen)


def prepare(module, config=None, dtype=torch.float32, device="cpu", frozen=True):
    """The module as the attack runs it: frozen, eval(), config attached."""
    from pcfa_amd import config as pcfa_config
    module = module.to(device=device, dtype=dtype).eval()
    for p in module.parameters():
        p.requires_grad_(not frozen)
    return pcfa_config.attach(module, config)


# --------------------------------------------------------------------------- evaluation and comparison
def evaluate(fn, inputs, diff, seed, dtype, device="cpu"):
    """fn(leaves) -> ordered dict of outputs.  Returns the outputs and, as "d_<input>", the gradients of
    sum_k <output_k, cotangent_k> with respect to every input named in `diff`; the cotangents are a function of
    (seed, position, shape) alone, so every execution of a case is differentiated along the same direction."""
    leaves = {}
    for k, v in inputs.items():
        v = v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)
        leaves[k] = v.clone().requires_grad_(True) if k in diff else v
    outs = fn(leaves)
    loss = 0
    for i, (k, o) in enumerate(outs.items()):
        g = torch.Generator().manual_seed(1009 * seed + i + 1)
        loss = loss + (o * torch.randn(tuple(o.shape), generator=g).to(o)).sum()
    grads = torch.autograd.grad(loss, [leaves[k] for k in diff])
    res = collections.OrderedDict((k, o.detach()) for k, o in outs.items())
    for k, g in zip(diff, grads):
        res["d_" + k] = g.detach()
    return res


def reference(case, seed, dtype=torch.float64):
    """(results, tape) of the restatement in `dtype` on the CPU from the fp32 parameter and input values."""
    module, x = materialise(case, seed)
    sd = {k: v.detach().to(dtype) for k, v in module.state_dict().items()}
    tape = Tape()
    return evaluate(lambda leaves: case.restate(sd, leaves, tape), x, case.diff, seed, dtype), tape


def first_clean_seed(case):
    """The first seed >= 0 whose float64 restatement keeps every margin, or None among MAX_SEEDS."""
    for seed in range(MAX_SEEDS):
        module, x = materialise(case, seed)
        sd = {k: v.detach().double() for k, v in module.state_dict().items()}
        tape = Tape()
        with torch.no_grad():
            case.restate(sd, {k: v.double() if v.is_floating_point() else v for k, v in x.items()}, tape)
        if tape.clean():
            return seed
    return None


def _f64(t):
    return t.detach().double().cpu()


def rel_l2(a, b):
    a, b = _f64(a), _f64(b)
    return float((a - b).norm() / b.norm())


def max_abs(a, b):
    return float((_f64(a) - _f64(b)).abs().max())


def distances(got, ref):
    """name -> (rel-L2, max|got - ref| / max|ref|) per tensor; (inf, inf) for a missing, misshapen or non-finite one."""
    out = collections.OrderedDict()
    for k, r in ref.items():
        g = got.get(k)
        if g is None or tuple(g.shape) != tuple(r.shape) or not bool(torch.isfinite(g).all()):
            out[k] = (math.inf, math.inf)
        else:
            out[k] = (rel_l2(g, r), max_abs(g, r) / float(_f64(r).abs().max()))
    return out


def failures(got, ref, rel=1e-11, ab=1e-11):
    """The tensors on which `got` misses `ref`: rel-L2 <= rel and max-abs <= ab * max|ref|, each tensor on its own."""
    return [k for k, (d, m) in distances(got, ref).items() if not (d <= rel and m <= ab)]


def bits_equal(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a)


# --------------------------------------------------------------------------- restatements: RAFT
def conv(sd, p, x, **kw):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], **kw)


def norm(sd, p, kind, x, eps=1e-5):
    """extractor.py:15-33: nn.BatchNorm2d in eval mode as its affine map, nn.InstanceNorm2d without affine."""
    if kind == "instance":
        return F.instance_norm(x, eps=eps)
    v = lambda name: sd[p + "." + name].view(1, -1, 1, 1)
    return (x - v("running_mean")) / torch.sqrt(v("running_var") + eps) * v("weight") + v("bias")


def residual_block(sd, p, x, kind, stride, tape, x_is_relu=False):
    """extractor.py:6-58.  x_is_relu: the block input is a ReLU output (every block inside an encoder)."""
    y = tape.relu(norm(sd, p + "norm1", kind, conv(sd, p + "conv1", x, stride=stride, padding=1)))
    y = tape.relu(norm(sd, p + "norm2", kind, conv(sd, p + "conv2", y, padding=1)))
    if stride != 1:
        x = norm(sd, p + "norm3", kind, conv(sd, p + "downsample.0", x, stride=stride))
    return tape.relu(x + y, sum_of_relus=x_is_relu and stride == 1)


def basic_encoder(sd, x, kind, tape):
    """extractor.py:118-192 in eval mode (a list input is concatenated by the caller)."""
    x = tape.relu(norm(sd, "norm1", kind, conv(sd, "conv1", x, stride=2, padding=3)))
    for layer, stride in ((1, 1), (2, 2), (3, 2)):
        x = residual_block(sd, "layer%d.0." % layer, x, kind, stride, tape, x_is_relu=True)
        x = residual_block(sd, "layer%d.1." % layer, x, kind, 1, tape, x_is_relu=True)
    return conv(sd, "conv2", x)


def corr_pyramid(fmap1, fmap2, levels=4):
    """corr.py:13-27,52-60."""
    b, d, h, w = fmap1.shape
    vol = torch.matmul(fmap1.view(b, d, h * w).transpose(1, 2), fmap2.view(b, d, h * w)) / math.sqrt(d)
    vol = vol.reshape(b * h * w, 1, h, w)
    pyramid = [vol]
    for _ in range(levels - 1):
        vol = F.avg_pool2d(vol, 2, stride=2)
        pyramid.append(vol)
    return pyramid


def bilinear_sampler(img, coords):
    """utils/utils.py:57-71: pixel coordinates, zero outside.  An axis of one pixel (the last level of an 8 x 12 map) makes
    the reference's 2 x / (W - 1) - 1 singular; one appended zero row / column is the same zero-padded sample."""
    if img.shape[-1] == 1 or img.shape[-2] == 1:
        img = F.pad(img, (0, int(img.shape[-1] == 1), 0, int(img.shape[-2] == 1)))
    h, w = img.shape[-2:]
    x, y = coords.split([1, 1], dim=-1)
    return F.grid_sample(img, torch.cat([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], dim=-1), align_corners=True)


def corr_lookup(pyramid, coords, r=4):
    """corr.py:29-50: meshgrid(dy, dx) is stacked onto (x, y), so the first window index moves x."""
    pts = coords.permute(0, 2, 3, 1)
    b, h, w, _ = pts.shape
    d = torch.linspace(-r, r, 2 * r + 1, dtype=coords.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out = []
    for i, vol in enumerate(pyramid):
        out.append(bilinear_sampler(vol, pts.reshape(b * h * w, 1, 1, 2) / 2 ** i + delta).view(b, h, w, -1))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2)


def motion_encoder(sd, p, flow, corr, tape):
    """update.py:79-101."""
    cor = tape.relu(conv(sd, p + "convc1", corr))
    cor = tape.relu(conv(sd, p + "convc2", cor, padding=1))
    flo = tape.relu(conv(sd, p + "convf1", flow, padding=3))
    flo = tape.relu(conv(sd, p + "convf2", flo, padding=1))
    out = tape.relu(conv(sd, p + "conv", torch.cat([cor, flo], dim=1), padding=1))
    return torch.cat([out, flow], dim=1)


def sepconv_gru(sd, p, h, x):
    """update.py:33-60."""
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(conv(sd, p + "convz" + n, hx, padding=pad))
        r = torch.sigmoid(conv(sd, p + "convr" + n, hx, padding=pad))
        q = torch.tanh(conv(sd, p + "convq" + n, torch.cat([r * h, x], dim=1), padding=pad))
        h = (1 - z) * h + z * q
    return h


def update_block(sd, p, net, inp, corr, flow, tape):
    """update.py:6-16,114-136."""
    motion = motion_encoder(sd, p + "encoder.", flow, corr, tape)
    net = sepconv_gru(sd, p + "gru.", net, torch.cat([inp, motion], dim=1))
    delta = conv(sd, p + "flow_head.conv2", tape.relu(conv(sd, p + "flow_head.conv1", net, padding=1)), padding=1)
    mask = .25 * conv(sd, p + "mask.2", tape.relu(conv(sd, p + "mask.0", net, padding=1)))
    return net, mask, delta


def upsample_flow(flow, mask):
    """raft.py:72-83."""
    n, _, h, w = flow.shape
    mask = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)


def grid(b, h, w, dtype):
    """utils/utils.py:74-77: channel 0 = x, channel 1 = y."""
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack([xs, ys], dim=0).to(dtype)[None].repeat(b, 1, 1, 1)


def raft_loop(sd, fmap1, fmap2, cnet_out, flow_init, iters, tape):
    """raft.py:99-144 behind the encoders: every iteration's up-sampled flow."""
    pyramid = corr_pyramid(fmap1, fmap2)
    net, inp = torch.split(cnet_out, [128, 128], dim=1)
    net, inp = torch.tanh(net), tape.relu(inp)
    b, _, h, w = fmap1.shape
    coords0 = grid(b, h, w, fmap1.dtype)
    coords1 = coords0 + flow_init
    ups = []
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_lookup(pyramid, coords1)
        net, mask, delta = update_block(sd, "update_block.", net, inp, corr, coords1 - coords0, tape)
        coords1 = coords1 + delta
        ups.append(upsample_flow(coords1 - coords0, mask))
    return ups


def gma_attention(sd, p, fmap):
    """gma.py:38-68, content only (position_only / position_and_content false, gma_config.json)."""
    b, c, h, w = fmap.shape
    heads = sd[p + "to_qk.weight"].shape[0] // (2 * 128)
    q, k = F.conv2d(fmap, sd[p + "to_qk.weight"]).chunk(2, dim=1)
    q = q.view(b, heads, 128, h * w).transpose(-1, -2) * 128 ** -0.5
    k = k.view(b, heads, 128, h * w).transpose(-1, -2)
    return torch.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1)


def gma_aggregate(sd, p, attn, fmap):
    """gma.py:86-115 (dim == heads * dim_head: no projection)."""
    b, c, h, w = fmap.shape
    v = F.conv2d(fmap, sd[p + "to_v.weight"])
    heads = v.shape[1] // 128
    out = torch.matmul(attn, v.view(b, heads, 128, h * w).transpose(-1, -2))
    return fmap + sd[p + "gamma"] * out.transpose(-1, -2).reshape(b, heads * 128, h, w)


def gma_update_block(sd, p, net, inp, corr, flow, attn, tape):
    """gma/update.py:112-139."""
    motion = motion_encoder(sd, p + "encoder.", flow, corr, tape)
    glob = gma_aggregate(sd, p + "aggregator.", attn, motion)
    net = sepconv_gru(sd, p + "gru.", net, torch.cat([inp, motion, glob], dim=1))
    delta = conv(sd, p + "flow_head.conv2", tape.relu(conv(sd, p + "flow_head.conv1", net, padding=1)), padding=1)
    mask = .25 * conv(sd, p + "mask.2", tape.relu(conv(sd, p + "mask.0", net, padding=1)))
    return net, mask, delta


def gma_loop(sd, fmap1, fmap2, cnet_out, flow_init, iters, tape):
    """gma/network.py:72-129 behind the encoders."""
    pyramid = corr_pyramid(fmap1, fmap2)
    net, inp = torch.split(cnet_out, [128, 128], dim=1)
    net, inp = torch.tanh(net), tape.relu(inp)
    attn = gma_attention(sd, "att.", inp)
    b, _, h, w = fmap1.shape
    coords0 = grid(b, h, w, fmap1.dtype)
    coords1 = coords0 + flow_init
    ups = []
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_lookup(pyramid, coords1)
        net, mask, delta = gma_update_block(sd, "update_block.", net, inp, corr, coords1 - coords0, attn, tape)
        coords1 = coords1 + delta
        ups.append(upsample_flow(coords1 - coords0, mask))
    return ups


def spynet_preprocess(x):
    """SpyNet.py:19-54 without pre_normalization."""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def spynet_basic(sd, p, x, tape):
    """SpyNet.py:56-84."""
    for i in range(0, 8, 2):
        x = tape.relu(conv(sd, "%s%d" % (p, i), x, padding=3))
    return conv(sd, p + "8", x, padding=3)


def spynet_warp(x, flow, tape):
    """SpyNet.py:86-102 (grid_sample's default: align_corners=False).  tape None: the flow is a constant (the zero flow of
    the coarsest level), nothing is differentiated through the coordinates.  Otherwise the margins are those of the
    sample's pixel ((v + 1) size - 1) / 2 to the nearest integer and of the unclamped v to the clamp at -1 and 1."""
    B, _, H, W = x.shape
    hor = torch.linspace(-1.0, 1.0, W, dtype=x.dtype).view(1, 1, 1, W).expand(B, 1, H, W)
    ver = torch.linspace(-1.0, 1.0, H, dtype=x.dtype).view(1, 1, H, 1).expand(B, 1, H, W)
    v = torch.cat([hor, ver], 1) + torch.cat([flow[:, 0:1] / ((W - 1.0) / 2.0), flow[:, 1:2] / ((H - 1.0) / 2.0)], 1)
    g = v.clamp(-1.0, 1.0)
    if tape is not None:
        for c, n in ((0, W), (1, H)):
            pix = ((g[:, c] + 1) * n - 1) / 2
            tape.distance((pix - torch.round(pix)).abs())
            tape.distance(torch.minimum((v[:, c] - 1).abs(), (v[:, c] + 1).abs()) * n / 2)
    return F.grid_sample(x, g.permute(0, 2, 3, 1), mode="bilinear", align_corners=False)


def spynet_forward(sd, first, second, nlevels, tape):
    """SpyNet.py:130-158 in eval mode (sides divisible by 2^(nlevels-1): the replicate pads never run)."""
    firsts, seconds = [spynet_preprocess(first)], [spynet_preprocess(second)]
    for _ in range(nlevels - 1):
        firsts.insert(0, F.avg_pool2d(firsts[0], kernel_size=2, stride=2))
        seconds.insert(0, F.avg_pool2d(seconds[0], kernel_size=2, stride=2))
    B, _, H, W = firsts[0].shape
    flow = torch.zeros((B, 2, H // 2, W // 2), dtype=first.dtype)
    for lvl in range(nlevels):
        up = F.interpolate(flow, scale_factor=2, mode="bilinear", align_corners=False) * 2.0
        warped = spynet_warp(seconds[lvl], up, tape if lvl else None)
        flow = spynet_basic(sd, "moduleBasic.%d.moduleBasic." % lvl, torch.cat([firsts[lvl], warped, up], 1), tape) + up
    return flow


def flownet_conv(sd, p, x, tape, stride=1):
    """FlowNet/submodules.py:7-19 (batchNorm=False): Conv2d(padding = (k - 1) // 2) + LeakyReLU(0.1)."""
    k = sd[p + ".0.weight"].shape[-1]
    return tape.leaky(conv(sd, p + ".0", x, stride=stride, padding=(k - 1) // 2))


def flownet_deconv(sd, p, x, tape):
    """FlowNet/submodules.py:36: ConvTranspose2d(4, 2, 1) + LeakyReLU(0.1)."""
    return tape.leaky(F.conv_transpose2d(x, sd[p + ".0.weight"], sd[p + ".0.bias"], stride=2, padding=1))


def flownet_s(sd, x, tape):
    """FlowNetS.py:53-95 in eval mode: flow2."""
    c2 = flownet_conv(sd, "conv2", flownet_conv(sd, "conv1", x, tape, 2), tape, 2)
    c3 = flownet_conv(sd, "conv3_1", flownet_conv(sd, "conv3", c2, tape, 2), tape)
    c4 = flownet_conv(sd, "conv4_1", flownet_conv(sd, "conv4", c3, tape, 2), tape)
    c5 = flownet_conv(sd, "conv5_1", flownet_conv(sd, "conv5", c4, tape, 2), tape)
    cat = flownet_conv(sd, "conv6_1", flownet_conv(sd, "conv6", c5, tape, 2), tape)
    for lvl, skip in ((6, c5), (5, c4), (4, c3), (3, c2)):
        flow = conv(sd, "predict_flow%d" % lvl, cat, padding=1)
        up = F.conv_transpose2d(flow, sd["upsampled_flow%d_to_%d.weight" % (lvl, lvl - 1)],
                                sd.get("upsampled_flow%d_to_%d.bias" % (lvl, lvl - 1)), stride=2, padding=1)
        cat = torch.cat((skip, flownet_deconv(sd, "deconv%d" % (lvl - 1), cat, tape), up), 1)
    return conv(sd, "predict_flow2", cat, padding=1)


def flownet_warp_block(x, flow, tape):
    """FlowNet2.py:128-134: Resample2d of image 2 (resample2d_kernel.cu:16-72: bilinear, each tap index clamped into the
    image -- at sample positions >= 0, which the case keeps, the border-replicating sample in pixel coordinates) and the
    ChannelNorm of the brightness error (channelnorm_kernel.cu:18-96).  The norm's backward is stated as the kernel has
    it, g x / (norm + 1e-9): the value is the plain square root, the 1e-9 enters the gradient alone."""
    B, _, H, W = x.shape
    xs = torch.arange(W, dtype=x.dtype).view(1, 1, W) + flow[:, 0]
    ys = torch.arange(H, dtype=x.dtype).view(1, H, 1) + flow[:, 1]
    for pix in (xs, ys):
        assert float(pix.detach().min()) >= 0
        tape.distance((pix - torch.round(pix)).abs())
    g = torch.stack((2 * xs / (W - 1) - 1, 2 * ys / (H - 1) - 1), dim=3)
    resampled = F.grid_sample(x[:, 3:], g, mode="bilinear", padding_mode="border", align_corners=True)
    diff = x[:, :3] - resampled
    n = torch.sqrt((diff.detach() ** 2).sum(1, keepdim=True))
    tape._pre(n)
    unit = diff.detach() / (n + 1e-9)
    return resampled, n + (diff * unit).sum(1, keepdim=True) - (diff.detach() * unit).sum(1, keepdim=True)


def smooth_flow(gen, b, h, w, amp=2.5):
    """A smooth flow of a few pixels with seeded phases."""
    ph = torch.rand(4, generator=gen) * 2 * math.pi
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    u = amp * torch.sin(2 * math.pi * xs / w + ph[0]) * torch.cos(math.pi * ys / h + ph[1]) + 0.37
    v = amp * 0.6 * torch.cos(2 * math.pi * ys / h + ph[2]) * torch.sin(math.pi * xs / w + ph[3]) - 0.21
    return torch.stack([u, v], dim=0)[None].repeat(b, 1, 1, 1).contiguous()


# --------------------------------------------------------------------------- restatements: PWC-Net
def conv_leaky(sd, p, x, tape, stride=1, dilation=1):
    """PWCNet.py:29-35: 3x3 Conv2d (padding = dilation) + LeakyReLU(0.1); parameter names "<p>.0.*"."""
    return tape.leaky(conv(sd, p + ".0", x, stride=stride, padding=dilation, dilation=dilation))


def pwc_pyramid_level(sd, x, bgr, tape):
    """PWCNet.py:231-246: one level of the feature pyramid (stride-2 layer and two stride-1 layers)."""
    if bgr:
        x = torch.stack((x[:, 2], x[:, 1], x[:, 0]), 1)
    x = conv_leaky(sd, "0", x, tape, stride=2)
    return conv_leaky(sd, "2", conv_leaky(sd, "1", x, tape), tape)


def pwc_context(sd, x, tape):
    """PWCNet.py:316-319: flow2 = predict_flow2(x) + dc_conv7(dc_conv6(.. dc_conv1(x)))."""
    flow = conv(sd, "predict_flow2", x, padding=1)
    y = x
    for i, d in enumerate((1, 2, 4, 8, 16, 1), start=1):
        y = conv_leaky(sd, "dc_conv%d" % i, y, tape, dilation=d)
    return flow + conv(sd, "dc_conv7", y, padding=1)


def pwc_warp(x, flo, tape):
    """PWCNet.py:166-206 (grid_sample's default: align_corners=False).  Margins: the sample sits at pixel
    ((v + 1) size - 1) / 2 of the zero-padded map; taps change at integers (the borders -1, 0, size - 1, size among them);
    the validity mask is a bilinear sample of ones, 1-Lipschitz in each pixel coordinate, compared with 0.0001 -- where it
    is exactly zero the sample lies outside the padded map and its way to the threshold leads over an integer, whose
    distance is already recorded."""
    B, C, H, W = x.shape
    v = grid(B, H, W, x.dtype) + flo
    vx = 2.0 * v[:, 0] / max(W - 1, 1) - 1.0
    vy = 2.0 * v[:, 1] / max(H - 1, 1) - 1.0
    vgrid = torch.stack((vx, vy), dim=3)
    out = F.grid_sample(x, vgrid, align_corners=False)
    mask = F.grid_sample(torch.ones_like(x), vgrid, align_corners=False)
    for pix in (((vx + 1) * W - 1) / 2, ((vy + 1) * H - 1) / 2):
        tape.distance((pix - torch.round(pix)).abs())
    m = mask[:, 0].detach()
    tape.distance(torch.where(m == 0, torch.ones_like(m), (m - 0.0001).abs()))
    return out * (mask >= 0.0001).to(x.dtype)


def pwc_cost_volume(f1, f2, tape):
    """PWCNet.py:45-58 (patch 9, kernel 1, stride 1, averaged over channels) and the leakyRELU that follows every call."""
    B, C, H, W = f1.shape
    p = F.pad(f2, (4, 4, 4, 4))
    out = torch.stack([(f1 * p[:, :, i:i + H, j:j + W]).sum(1) for i in range(9) for j in range(9)], 1) / C
    return tape.leaky(out, zero_padded=True)


def deconv(sd, p, x):
    """PWCNet.py:42-43: ConvTranspose2d(in, out, 4, 2, 1)."""
    return F.conv_transpose2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=2, padding=1)


def pwc_decoder_level(sd, lvl, f1, f2, up_flow, up_feat, scale, tape):
    """PWCNet.py:249-316 for one level: (the dense block's output, its flow)."""
    if lvl == 6:
        x = pwc_cost_volume(f1, f2, tape)
    else:
        x = torch.cat((pwc_cost_volume(f1, pwc_warp(f2, up_flow * scale, tape), tape), f1, up_flow, up_feat), 1)
    for i in range(5):
        x = torch.cat((conv_leaky(sd, "conv%d_%d" % (lvl, i), x, tape), x), 1)
    return x, conv(sd, "predict_flow%d" % lvl, x, padding=1)


_PWC_SCALE = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}


def pwc_forward(sd, im1, im2, tape):
    """PWCNet.py:227-330 in eval mode."""
    def pyramid(im):
        feats, x = [], torch.stack((im[:, 2], im[:, 1], im[:, 0]), 1)
        for lvl in range(1, 7):
            first, second = ("aa", "a") if lvl == 6 else ("a", "aa")
            x = conv_leaky(sd, "conv%d%s" % (lvl, first), x, tape, stride=2)
            x = conv_leaky(sd, "conv%db" % lvl, conv_leaky(sd, "conv%d%s" % (lvl, second), x, tape), tape)
            feats.append(x)
        return feats

    c1, c2 = pyramid(im1), pyramid(im2)
    up_flow = up_feat = None
    for lvl in (6, 5, 4, 3, 2):
        x, flow = pwc_decoder_level(sd, lvl, c1[lvl - 1], c2[lvl - 1], up_flow, up_feat, _PWC_SCALE.get(lvl), tape)
        if lvl > 2:
            up_flow, up_feat = deconv(sd, "deconv%d" % lvl, flow), deconv(sd, "upfeat%d" % lvl, x)
    y = x
    for i, d in enumerate((1, 2, 4, 8, 16, 1), start=1):
        y = conv_leaky(sd, "dc_conv%d" % i, y, tape, dilation=d)
    flow = flow + conv(sd, "dc_conv7", y, padding=1)
    return 20 * F.interpolate(flow, scale_factor=4, mode="bilinear", align_corners=False)


# --------------------------------------------------------------------------- cases
# The committed seeds: first_clean_seed(case) of each, found in float64 on the CPU; the CPU tier re-derives them.
SEEDS = {
    "resblock-instance-s1-2x12x16": 0, "resblock-instance-s2-2x12x16": 0, "resblock-batch-s1-2x12x16": 0,
    "resblock-batch-s2-2x12x16": 0, "resblock-instance-s1-1x9x14": 0, "resblock-instance-s2-1x9x14": 0,
    "resblock-batch-s1-1x9x14": 1, "resblock-batch-s2-1x9x14": 0,
    "encoder-instance-split-32x48": 1, "encoder-instance-pair-32x48": 1, "encoder-batch-single-32x48": 4,
    "update-b1-mask-8x12": 0, "update-b1-nomask-8x12": 0, "update-b2-mask-8x12": 0, "update-b2-nomask-8x12": 0,
    "raftloop-test-8x12": 1, "raftloop-train-8x12": 1,
    "pwcpyr-l1-20x32": 0, "pwcpyr-l1-20x36": 0, "pwcpyr-l1-20x30": 0,
    "pwcpyr-l3-20x32": 0, "pwcpyr-l3-20x36": 1, "pwcpyr-l3-20x30": 1,
    "pwcctx-16x32": 0, "pwcctx-16x24": 2, "pwcctx-8x12": 0,
    "pwcdec-l5-1x6x8": 0, "pwcdec-l5-1x5x7": 0, "pwcdec-l5-2x6x8": 3,
    "pwcdec-l2-1x6x8": 0, "pwcdec-l2-1x5x7": 0, "pwcdec-l2-2x6x8": 0,
    "pwcdec-l6-1x6x8": 0, "pwcdec-l6-1x5x7": 0, "pwcdec-l6-2x6x8": 0,
    "pwcnet-64x64": 30,
    "gma-attnagg-8x12": 0, "gma-attnagg-9x15": 0, "gma-update-mask-8x12": 0, "gma-update-nomask-8x12": 0,
    "gmaloop-test-8x12": 8, "gmaloop-train-8x12": 8,
    "spybasic-8x12": 0, "spynet2-16x24": 6,
    "flownets-64x128": 2, "flownet2-warp-64x128": 0,
}


class Case:
    """One composite at one shape.  seed: the committed first margin-clean seed (tests re-derive / re-assert it)."""
    diff = ("x",)

    def __init__(self, name):
        self.name, self.seed = name, SEEDS.get(name)

    def __repr__(self):
        return self.name


class ResBlock(Case):
    def __init__(self, kind, stride, B, H, W):
        super().__init__("resblock-%s-s%d-%dx%dx%d" % (kind, stride, B, H, W))
        self.kind, self.stride, self.shape = kind, stride, (B, 64, H, W)

    def make_module(self):
        from pcfa_amd.nets import raft
        return raft.ResidualBlock(64, 64 if self.stride == 1 else 96, self.kind, stride=self.stride)

    def make_inputs(self, gen):
        return {"x": torch.randn(self.shape, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(out=residual_block(sd, "", x["x"], self.kind, self.stride, tape))

    def run(self, module, x):
        return collections.OrderedDict(out=module(x["x"]))


class Encoder(Case):
    """mode: "split" (one batch holding both images, split=1), "pair" (a pair of tensors), "single"."""

    def __init__(self, kind, mode, H=32, W=48):
        super().__init__("encoder-%s-%s-%dx%d" % (kind, mode, H, W))
        self.kind, self.mode, self.hw = kind, mode, (H, W)
        self.diff = ("x1", "x2") if mode == "pair" else ("x",)

    def make_module(self):
        from pcfa_amd.nets import raft
        return raft.BasicEncoder(output_dim=256, norm_fn=self.kind)

    def make_inputs(self, gen):
        img = lambda b: 2 * torch.rand((b, 3) + self.hw, generator=gen) - 1
        if self.mode == "pair":
            return {"x1": img(1), "x2": img(1)}
        return {"x": img(2 if self.mode == "split" else 1)}

    def restate(self, sd, x, tape):
        if self.mode == "single":
            return collections.OrderedDict(out=basic_encoder(sd, x["x"], self.kind, tape))
        y = basic_encoder(sd, torch.cat([x["x1"], x["x2"]], 0) if self.mode == "pair" else x["x"], self.kind, tape)
        return collections.OrderedDict(out1=y[:1], out2=y[1:])

    def run(self, module, x):
        if self.mode == "single":
            return collections.OrderedDict(out=module(x["x"]))
        a, b = module(x["x"], split=1) if self.mode == "split" else module((x["x1"], x["x2"]))
        return collections.OrderedDict(out1=a, out2=b)


class UpdateBlock(Case):
    """BasicUpdateBlock.forward for one iteration, gru_ctx from precompute / per_iteration(.., 1), a LookupRef on a real
    correlation block over leaf feature maps; coordinates = grid + the (smooth) flow."""
    diff = ("net", "inp", "fmap1", "fmap2", "flow")

    def __init__(self, B, want_mask, H=8, W=12):
        super().__init__("update-b%d-%s-%dx%d" % (B, "mask" if want_mask else "nomask", H, W))
        self.B, self.want_mask, self.hw = B, want_mask, (H, W)

    def make_module(self):
        from pcfa_amd.nets import raft
        return raft.BasicUpdateBlock(4, 4, hidden_dim=128)

    def make_inputs(self, gen):
        B, (H, W) = self.B, self.hw
        r = lambda c: torch.randn((B, c, H, W), generator=gen)
        return {"net": torch.tanh(r(128)), "inp": torch.relu(r(128)), "fmap1": r(256), "fmap2": r(256),
                "flow": smooth_flow(gen, B, H, W)}

    def restate(self, sd, x, tape):
        flow = x["flow"]
        coords = grid(self.B, *self.hw, flow.dtype) + flow.detach()
        corr = corr_lookup(corr_pyramid(x["fmap1"], x["fmap2"]), coords)
        net, mask, delta = update_block(sd, "", x["net"], x["inp"], corr, flow, tape)
        out = collections.OrderedDict(net=net, delta_flow=delta)
        if self.want_mask:
            out["mask"] = mask
        return out

    def run(self, module, x):
        from pcfa_amd import ops
        from pcfa_amd.config import cfg
        from pcfa_amd.nets import raft
        c, o = cfg(module), ops.get()
        if c.corr == "on_demand":
            corr_fn = o.OnDemandCorrBlock(x["fmap1"], x["fmap2"], num_levels=4, radius=4, lookup=c.ondemand_lookup)
        else:
            corr_fn = o.CorrBlock(x["fmap1"], x["fmap2"], num_levels=4, radius=4, bwd_windows=c.pyramid_bwd_windows,
                                  **raft.mfma_kw(c))
        flow = x["flow"]
        coords = raft.coords_grid(self.B, *self.hw, flow.device, flow.dtype) + flow.detach()
        gru = module.gru
        ctx = gru.per_iteration(gru.precompute(x["inp"]), 1)[0] if gru.frozen() else None
        net, mask, delta = module(x["net"], x["inp"], raft.LookupRef(corr_fn, coords), flow, want_mask=self.want_mask,
                                  gru_ctx=ctx)
        out = collections.OrderedDict(net=net, delta_flow=delta)
        if self.want_mask:
            out["mask"] = mask
        else:
            assert mask is None
        return out


class _Leaf(nn.Module):
    """Stands in for an encoder: returns the leaf tensors the test differentiates."""
    value = None

    def forward(self, x, split=None):
        return self.value


class RaftLoop(Case):
    """RAFT.forward behind its encoders: fnet / cnet replaced by stubs that return leaf tensors; iters = 3, non-zero
    flow_init.  test_mode scores the last flow_up, training mode all three predictions."""
    diff = ("fmap1", "fmap2", "cnet_out")
    ITERS = 3

    def __init__(self, test_mode, H=8, W=12):
        super().__init__("raftloop-%s-%dx%d" % ("test" if test_mode else "train", H, W))
        self.test_mode, self.hw = test_mode, (H, W)

    def make_module(self):
        from pcfa_amd.nets import raft
        model = raft.RAFT()
        model.fnet, model.cnet = _Leaf(), _Leaf()
        return model

    def make_inputs(self, gen):
        H, W = self.hw
        r = lambda c: torch.randn((1, c, H, W), generator=gen)
        img = lambda: 255 * torch.rand((1, 3, 8 * H, 8 * W), generator=gen)
        return {"fmap1": r(256), "fmap2": r(256), "cnet_out": r(256), "flow_init": smooth_flow(gen, 1, H, W, 1.5),
                "image1": img(), "image2": img()}

    def restate(self, sd, x, tape):
        ups = raft_loop(sd, x["fmap1"], x["fmap2"], x["cnet_out"], x["flow_init"], self.ITERS, tape)
        if self.test_mode:
            return collections.OrderedDict(flow_up=ups[-1])
        return collections.OrderedDict(("flow_up%d" % i, u) for i, u in enumerate(ups))

    def run(self, module, x):
        module.fnet.value, module.cnet.value = (x["fmap1"], x["fmap2"]), x["cnet_out"]
        out = module(x["image1"], x["image2"], iters=self.ITERS, flow_init=x["flow_init"], test_mode=self.test_mode)
        if self.test_mode:
            return collections.OrderedDict(flow_up=out[1])
        assert len(out) == self.ITERS
        return collections.OrderedDict(("flow_up%d" % i, u) for i, u in enumerate(out))


_PWC_PYRAMID = {1: (3, 16), 3: (32, 64)}


class PwcPyramid(Case):
    """_chain([conv_a, conv_aa, conv_b], x, bgr_input=..) of one pyramid level on the two-image batch."""

    def __init__(self, level, H, W):
        super().__init__("pwcpyr-l%d-%dx%d" % (level, H, W))
        self.level, self.hw = level, (H, W)

    def make_module(self):
        from pcfa_amd.nets import pwcnet
        cin, cout = _PWC_PYRAMID[self.level]
        return nn.ModuleList([pwcnet.conv(cin, cout, stride=2), pwcnet.conv(cout, cout), pwcnet.conv(cout, cout)])

    def make_inputs(self, gen):
        return {"x": torch.randn((2, _PWC_PYRAMID[self.level][0]) + self.hw, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(out=pwc_pyramid_level(sd, x["x"], self.level == 1, tape))

    def fold_bgr(self, module, x):
        """PWCDCNet.forward's decision: RGB -> BGR in conv1a's weights where that layer runs on the operator table."""
        from pcfa_amd.config import cfg
        return self.level == 1 and cfg(module[0]).pwc_fold_glue and module[0].kind(x) is not None

    def run(self, module, x):
        from pcfa_amd.nets import pwcnet
        x = x["x"]
        fold = self.fold_bgr(module, x)
        if self.level == 1 and not fold:
            x = torch.stack((x[:, 2], x[:, 1], x[:, 0]), 1)
        return collections.OrderedDict(out=pwcnet._chain(list(module), x, bgr_input=fold))


class _Context(nn.Module):
    def __init__(self):
        super().__init__()
        from pcfa_amd.nets import pwcnet
        self.dc_conv1 = pwcnet.conv(565, 128, padding=1, dilation=1)
        self.dc_conv2 = pwcnet.conv(128, 128, padding=2, dilation=2)
        self.dc_conv3 = pwcnet.conv(128, 128, padding=4, dilation=4)
        self.dc_conv4 = pwcnet.conv(128, 96, padding=8, dilation=8)
        self.dc_conv5 = pwcnet.conv(96, 64, padding=16, dilation=16)
        self.dc_conv6 = pwcnet.conv(64, 32, padding=1, dilation=1)
        self.dc_conv7 = pwcnet.predict_flow(32)
        self.predict_flow2 = pwcnet.predict_flow(565)

    def chain(self):
        return [getattr(self, "dc_conv%d" % i) for i in range(1, 7)]


class PwcContext(Case):
    """_chain(dc_conv1..6, x, skip_first=True) + predict_flow2 on the alias + dc_conv7, summed."""

    def __init__(self, H, W):
        super().__init__("pwcctx-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        return _Context()

    def make_inputs(self, gen):
        return {"x": torch.randn((1, 565) + self.hw, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(flow=pwc_context(sd, x["x"], tape))

    def run(self, module, x):
        from pcfa_amd.nets import pwcnet
        from pcfa_amd.config import cfg
        x, c = x["x"], cfg(module)
        if c.pwc_fold_glue and c.defer_leaky and module.dc_conv1.kind(x) == "conv3x3":
            ctx, alias = pwcnet._chain(module.chain(), x, skip_first=True)
            flow = module.predict_flow2(alias)
        else:   # (PWCDCNet.forward's other branch: trainable weights, or either switch off)
            flow = module.predict_flow2(x)
            ctx = pwcnet._chain(module.chain(), x)
        return collections.OrderedDict(flow=flow + module.dc_conv7(ctx))


class PwcDecoder(Case):
    """warp(f2, up_flow, scale) -> _cost_volume -> _decode(lvl, corr, f1, up_flow, up_feat) -> _flow_head -> deconv /
    upfeat for one level (level 6: no warp, a single part; level 2: predict_flow2 on the decoded features)."""

    def __init__(self, level, B, H, W):
        super().__init__("pwcdec-l%d-%dx%dx%d" % (level, B, H, W))
        self.level, self.B, self.hw = level, B, (H, W)
        self.diff = ("f1", "f2") if level == 6 else ("f1", "f2", "up_flow", "up_feat")

    def make_module(self):
        from pcfa_amd.nets import pwcnet
        return pwcnet.PWCDCNet()

    def make_inputs(self, gen):
        B, (H, W) = self.B, self.hw
        c = {6: 196, 5: 128, 2: 32}[self.level]
        x = {"f1": torch.randn((B, c, H, W), generator=gen), "f2": torch.randn((B, c, H, W), generator=gen)}
        if self.level != 6:   # a flow whose scaled version moves the samples by up to two pixels
            x["up_flow"] = smooth_flow(gen, B, H, W, 2.0 / _PWC_SCALE[self.level])
            x["up_feat"] = torch.randn((B, 2, H, W), generator=gen)
        return x

    def _outputs(self, feat, flow, up):
        if self.level == 2:
            return collections.OrderedDict(feat=feat, flow=flow)
        return collections.OrderedDict(flow=flow, up_flow=up("deconv%d" % self.level, flow),
                                       up_feat=up("upfeat%d" % self.level, feat))

    def restate(self, sd, x, tape):
        feat, flow = pwc_decoder_level(sd, self.level, x["f1"], x["f2"], x.get("up_flow"), x.get("up_feat"),
                                       _PWC_SCALE.get(self.level), tape)
        return self._outputs(feat, flow, lambda name, t: deconv(sd, name, t))

    def run(self, model, x):
        lvl = self.level
        if lvl == 6:
            feat = model._decode(6, model._cost_volume(x["f1"], x["f2"]))
        else:
            corr = model._cost_volume(x["f1"], model.warp(x["f2"], x["up_flow"], _PWC_SCALE[lvl]))
            feat = model._decode(lvl, corr, x["f1"], x["up_flow"], x["up_feat"])
        if lvl == 2:
            flow = model.predict_flow2(feat)
        else:
            flow, feat = model._flow_head(lvl, feat)
        return self._outputs(feat, flow, lambda name, t: getattr(model, name)(t))


class PwcForward(Case):
    """PWCDCNet.forward end to end, eval."""
    diff = ("im1", "im2")

    def __init__(self, H, W):
        super().__init__("pwcnet-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        from pcfa_amd.nets import pwcnet
        return pwcnet.PWCDCNet()

    def make_inputs(self, gen):
        return {"im1": torch.rand((1, 3) + self.hw, generator=gen), "im2": torch.rand((1, 3) + self.hw, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(flow=pwc_forward(sd, x["im1"], x["im2"], tape))

    def run(self, model, x):
        return collections.OrderedDict(flow=model(x["im1"], x["im2"]))


class _AttnAgg(nn.Module):
    def __init__(self):
        super().__init__()
        from argparse import Namespace
        from pcfa_amd.nets import gma
        args = Namespace(position_only=False, position_and_content=False, num_heads=1)
        self.att = gma.Attention(args=args, dim=128, heads=1, max_pos_size=160, dim_head=128)
        self.aggregator = gma.Aggregate(args=args, dim=128, dim_head=128, heads=1)


def _attn_share(module):
    """RAFTGMA.forward's choice of the book-keeping object for the shared attention gradient."""
    from pcfa_amd import ops
    from pcfa_amd.config import cfg
    from pcfa_amd.nets import gma
    o = ops.get()
    return o.AttnGradShare(cfg(module).gma_gemm, cfg(module).mfma) if hasattr(o, "AttnGradShare") else gma._SharedAttnGrad()


class GmaAttnAgg(Case):
    """Attention on the context features, then Aggregate for three iterations' motion features sharing that one attention
    (its gradient formed once, through _SharedAttnGrad / AttnGradShare)."""
    diff = ("inp", "m0", "m1", "m2")

    def __init__(self, H, W):
        super().__init__("gma-attnagg-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        return _AttnAgg()

    def make_inputs(self, gen):
        r = lambda: torch.randn((1, 128) + self.hw, generator=gen)
        return {"inp": torch.relu(r()), "m0": r(), "m1": r(), "m2": r()}

    def restate(self, sd, x, tape):
        attn = gma_attention(sd, "att.", x["inp"])
        return collections.OrderedDict(("agg%d" % i, gma_aggregate(sd, "aggregator.", attn, x["m%d" % i])) for i in range(3))

    def run(self, module, x):
        attn, shared = module.att(x["inp"]), _attn_share(module)
        return collections.OrderedDict(("agg%d" % i, module.aggregator(attn, x["m%d" % i], shared)) for i in range(3))


class GmaUpdate(Case):
    """GMAUpdateBlock.forward for one iteration on a given attention (from Attention on the context features)."""
    diff = ("net", "inp", "fmap1", "fmap2", "flow")

    def __init__(self, want_mask, H=8, W=12):
        super().__init__("gma-update-%s-%dx%d" % ("mask" if want_mask else "nomask", H, W))
        self.want_mask, self.hw = want_mask, (H, W)

    def make_module(self):
        from argparse import Namespace
        from pcfa_amd.nets import gma
        model = gma.RAFTGMA(Namespace(position_only=False, position_and_content=False, num_heads=1))
        model.fnet, model.cnet = _Leaf(), _Leaf()
        return model

    def make_inputs(self, gen):
        H, W = self.hw
        r = lambda c: torch.randn((1, c, H, W), generator=gen)
        return {"net": torch.tanh(r(128)), "inp": torch.relu(r(128)), "fmap1": r(256), "fmap2": r(256),
                "flow": smooth_flow(gen, 1, H, W)}

    def _out(self, net, mask, delta):
        out = collections.OrderedDict(net=net, delta_flow=delta)
        if self.want_mask:
            out["mask"] = mask
        return out

    def restate(self, sd, x, tape):
        flow = x["flow"]
        coords = grid(1, *self.hw, flow.dtype) + flow.detach()
        corr = corr_lookup(corr_pyramid(x["fmap1"], x["fmap2"]), coords)
        attn = gma_attention(sd, "att.", x["inp"])
        return self._out(*gma_update_block(sd, "update_block.", x["net"], x["inp"], corr, flow, attn, tape))

    def run(self, model, x):
        from pcfa_amd import ops
        from pcfa_amd.config import cfg
        from pcfa_amd.nets import raft
        c, o = cfg(model), ops.get()
        if c.corr == "on_demand":
            corr_fn = o.OnDemandCorrBlock(x["fmap1"], x["fmap2"], num_levels=4, radius=4, lookup=c.ondemand_lookup)
        else:
            corr_fn = o.CorrBlock(x["fmap1"], x["fmap2"], num_levels=4, radius=4, bwd_windows=c.pyramid_bwd_windows,
                                  **raft.mfma_kw(c))
        flow = x["flow"]
        coords = raft.coords_grid(1, *self.hw, flow.device, flow.dtype) + flow.detach()
        ub = model.update_block
        ctx = ub.gru.per_iteration(ub.gru.precompute(x["inp"]), 1)[0] if ub.gru.frozen() else None
        net, mask, delta = ub(x["net"], x["inp"], raft.LookupRef(corr_fn, coords), flow, model.att(x["inp"]),
                              want_mask=self.want_mask, gru_ctx=ctx, attn_grad=_attn_share(model))
        assert self.want_mask or mask is None
        return self._out(net, mask, delta)


class GmaLoop(RaftLoop):
    """RAFTGMA.forward behind its encoders (the stubs of RaftLoop)."""

    def __init__(self, test_mode, H=8, W=12):
        Case.__init__(self, "gmaloop-%s-%dx%d" % ("test" if test_mode else "train", H, W))
        self.test_mode, self.hw = test_mode, (H, W)

    make_module = GmaUpdate.make_module

    def restate(self, sd, x, tape):
        ups = gma_loop(sd, x["fmap1"], x["fmap2"], x["cnet_out"], x["flow_init"], self.ITERS, tape)
        if self.test_mode:
            return collections.OrderedDict(flow_up=ups[-1])
        return collections.OrderedDict(("flow_up%d" % i, u) for i, u in enumerate(ups))


class SpyBasic(Case):
    """Basic(x, addend): the five 7x7 layers and the caller's `+ up`."""
    diff = ("x", "addend")

    def __init__(self, H, W):
        super().__init__("spybasic-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        from pcfa_amd.nets import spynet
        return spynet.Basic(0)

    def make_inputs(self, gen):
        return {"x": torch.randn((1, 8) + self.hw, generator=gen), "addend": torch.randn((1, 2) + self.hw, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(flow=spynet_basic(sd, "moduleBasic.", x["x"], tape) + x["addend"])

    def run(self, module, x):
        return collections.OrderedDict(flow=module(x["x"], x["addend"]))


class SpyTwoLevels(Case):
    """Network.forward over two pyramid levels (warp -> Basic -> up-sampled flow addend), eval."""
    diff = ("first", "second")

    def __init__(self, H, W):
        super().__init__("spynet2-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        from pcfa_amd.nets import spynet
        return spynet.Network(nlevels=2)

    def make_inputs(self, gen):
        return {k: torch.rand((1, 3) + self.hw, generator=gen) for k in ("first", "second")}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(flow=spynet_forward(sd, x["first"], x["second"], 2, tape))

    def run(self, module, x):
        return collections.OrderedDict(flow=module(x["first"], x["second"]))


class FlowNetSCase(Case):
    """FlowNetS.forward: the encoder and _Refinement._decode."""

    def __init__(self, H, W):
        super().__init__("flownets-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        from pcfa_amd.nets import flownet2
        return flownet2.FlowNetS()

    def make_inputs(self, gen):
        return {"x": torch.randn((1, 12) + self.hw, generator=gen)}

    def restate(self, sd, x, tape):
        return collections.OrderedDict(flow2=flownet_s(sd, x["x"], tape))

    def run(self, module, x):
        out = module(x["x"])
        assert len(out) == 1
        return collections.OrderedDict(flow2=out[0])


class _WarpBlock(nn.Module):
    """FlowNet2._warp_block needs no parameter: the method is borrowed, the network is not built."""

    def forward(self, x, flow):
        from pcfa_amd.config import cfg
        from pcfa_amd.nets import flownet2
        return flownet2.FlowNet2._warp_block(self, x, flow, cfg(self).flownet2_ops == "hip" and x.is_cuda)


class FlowNetWarp(Case):
    """FlowNet2._warp_block: Resample2d (its fixed-point backward under flownet2_ops = "hip") and ChannelNorm of the
    brightness error.  The flow moves every sample by 1.05 .. 1.45 pixels in x and 0.05 .. 0.45 in y: positions stay
    non-negative (where the reference's backward kernel is the derivative of its forward) and a twentieth of a pixel
    from every integer by construction -- 16 384 random coordinates would never all keep 2^-10."""
    diff = ("x", "flow")

    def __init__(self, H, W):
        super().__init__("flownet2-warp-%dx%d" % (H, W))
        self.hw = (H, W)

    def make_module(self):
        return _WarpBlock()

    def make_inputs(self, gen):
        H, W = self.hw
        ph = torch.rand(2, generator=gen) * 2 * math.pi
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        wave = 2 * math.pi * (xs / W + ys / H)
        flow = torch.stack([1.25 + 0.2 * torch.sin(wave + ph[0]), 0.25 + 0.2 * torch.cos(wave + ph[1])], 0)[None]
        return {"x": torch.randn((1, 6, H, W), generator=gen), "flow": flow.contiguous()}

    def restate(self, sd, x, tape):
        resampled, norm_diff = flownet_warp_block(x["x"], x["flow"], tape)
        return collections.OrderedDict(resampled=resampled, norm_diff=norm_diff)

    def run(self, module, x):
        resampled, norm_diff = module(x["x"], x["flow"])
        return collections.OrderedDict(resampled=resampled, norm_diff=norm_diff)


RESBLOCKS = [ResBlock(kind, stride, B, H, W) for (B, H, W) in ((2, 12, 16), (1, 9, 14))
             for kind in ("instance", "batch") for stride in (1, 2)]
ENCODERS = [Encoder("instance", "split"), Encoder("instance", "pair"), Encoder("batch", "single")]
UPDATES = [UpdateBlock(B, want_mask) for B in (1, 2) for want_mask in (True, False)]
LOOPS = [RaftLoop(True), RaftLoop(False)]
PYRAMIDS = [PwcPyramid(level, 20, W) for level in (1, 3) for W in (32, 36, 30)]
CONTEXTS = [PwcContext(16, 32), PwcContext(16, 24), PwcContext(8, 12)]
DECODERS = [PwcDecoder(level, B, H, W) for level in (5, 2, 6) for (B, H, W) in ((1, 6, 8), (1, 5, 7), (2, 6, 8))]
FORWARDS = [PwcForward(64, 64)]
GMA_ATTN = [GmaAttnAgg(8, 12), GmaAttnAgg(9, 15)]
GMA_UPDATES = [GmaUpdate(True), GmaUpdate(False)]
GMA_LOOPS = [GmaLoop(True), GmaLoop(False)]
SPYNET = [SpyBasic(8, 12), SpyTwoLevels(16, 24)]
FLOWNET2 = [FlowNetSCase(64, 128), FlowNetWarp(64, 128)]
CASES = (RESBLOCKS + ENCODERS + UPDATES + LOOPS + GMA_ATTN + GMA_UPDATES + GMA_LOOPS + PYRAMIDS + CONTEXTS + DECODERS
         + FORWARDS + SPYNET + FLOWNET2)
BY_NAME = {c.name: c for c in CASES}
