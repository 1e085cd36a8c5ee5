"""nn.conv2d and nn.ResNet on their own, at the shapes of gin/papers/icml2020/pretrain_model.gin's front end (log-mel [32, 125, 229]):
the 3 x 3 bottleneck convolution at [32, 125, 58, 32] -> 32 stride (1, 1) and [32, 125, 58, 64] -> 64 stride (1, 2), the 7 x 7 stem at
[32, 125, 229, 1] -> 64 stride (1, 2), the 1 x 1 convolutions of a residual layer against torch.matmul, the parts of one residual
layer, and ResNet('small') on [32, 125, 229, 1] - forward and forward + backward, on the kernel of csrc/conv2d.hip and, beside it,
the framework's route for a channel-last tensor (the thing compared against, not product code) on the same GPU in the same session:

  conv2d   F.relu, a permute to channel-first, F.pad with TF's 'same' rule, F.conv2d - MIOpen - and a permute back,

and the same model assembled from those ops, F.layer_norm and the same max pool, on the same weights.

    python tools/bench_resnet.py [out.json]

Warm clocks, medians of five timed loops (host wall clock around synchronised loops); one JSON line at the end.  Beside each
convolution: the HBM floor of one read of its input and one write of its output (8 TB/s).  Per residual layer: the time of its
parts - the three convolutions, the three normalisations - and the share spent outside the convolutions."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import ddsp_amd as ddsp  # noqa: F401
from ddsp_amd import build
from ddsp_amd.training import nn
build.build()

BATCH, FRAMES, BINS = 32, 125, 229
DEV = 'cuda'


def timed(fn, steps, repeats=5):
  for _ in range(2): fn()
  t_settle = time.perf_counter()
  while time.perf_counter() - t_settle < 0.05:    # the GPU needs ~20 ms of load to reach its sustained clock
    fn()
    torch.cuda.synchronize()
  out = []
  for _ in range(repeats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / steps)
  return [statistics.median(out) * 1e6, min(out) * 1e6, max(out) * 1e6]


def no_grad(fn):
  def run():
    with torch.no_grad(): fn()
  return run


# ---- the framework's route -------------------------------------------------------------------------------------------------------
def conv2d_route(x, kernel, bias, strides, relu=True):
  """x [b, h, w, ci], kernel [kh, kw, ci, co]."""
  a = F.relu(x) if relu else x
  (_, top, bottom), (_, left, right) = (nn.same_padding(n, k, s) for n, k, s in zip(x.shape[1:3], kernel.shape[:2], strides))
  padded = F.pad(a.permute(0, 3, 1, 2), (left, right, top, bottom))
  return F.conv2d(padded, kernel.permute(3, 2, 0, 1), bias, stride=strides).permute(0, 2, 3, 1).contiguous()


def framework_resnet(net):
  norm = lambda n, x: F.layer_norm(x, x.shape[1:], eps=1e-5) * n.scale + n.shift          # 'layer': moments over h, w and the channels
  conv = lambda c, x, relu: conv2d_route(x, c.kernel, c.bias, c.strides, relu)

  def layer(l, x):
    r = x
    x = F.relu(norm(l.norm_input, x))
    if l.shortcut:
      r = conv(l.conv_proj, x, False)
    x = conv(l.bottleneck[0], x, False)
    for block in l.bottleneck[1:]:
      x = conv(block.conv, norm(block.norm, x), True)
    return x + r

  def stack(s, x):
    for l in s.layers[:-1]:
      x = layer(l, x)
    return F.relu(norm(s.layers[-1], x))

  def run(x):
    stem, pool, first, second = net.layers
    return stack(second, stack(first, pool(conv(stem, x, False))))
  return run


result = {'workload': "the convolutions of nn.ResNet at the icml2020 front end's shapes and ResNet('small') on [32, 125, 229, 1]: the kernel of "
                      'csrc/conv2d.hip and the framework route (F.relu, F.pad, F.conv2d on the permuted tensor)',
          'note': 'timings are [median, min, max] in microseconds per call, host wall clock around synchronised loops; hbm_floor_us: one '
                  'read of the input and one write of the output at 8 TB/s',
          'convolutions': {}, 'one_by_one': {}, 'residual_layer_parts': {}, 'resnet_small': {}}
torch.manual_seed(0)


def operands(shape, ch_out, kh, kw, strides):
  b, h, w, ch_in = shape
  x = torch.randn(*shape, device=DEV, requires_grad=True)
  kernel = (torch.randn(kh, kw, ch_in, ch_out, device=DEV) * (2.0 / (kh * kw * ch_in)) ** 0.5).requires_grad_(True)
  bias = (0.1 * torch.randn(ch_out, device=DEV)).requires_grad_(True)
  out = (b, nn.same_padding(h, kh, strides[0])[0], nn.same_padding(w, kw, strides[1])[0], ch_out)
  return x, kernel, bias, torch.randn(*out, device=DEV)


# ---- single convolutions -----------------------------------------------------------------------------------------------------------
for name, shape, ch_out, k, strides, relu, steps in (('bottleneck_3x3_32_s1', (BATCH, FRAMES, 58, 32), 32, 3, (1, 1), True, 20),
                                                    ('bottleneck_3x3_64_s2', (BATCH, FRAMES, 58, 64), 64, 3, (1, 2), True, 20),
                                                    ('stem_7x7', (BATCH, FRAMES, BINS, 1), 64, 7, (1, 2), False, 10)):
  x, kernel, bias, cot = operands(shape, ch_out, k, k, strides)
  leaves = [x, kernel, bias]
  row = {'x': list(shape), 'ch_out': ch_out, 'kernel': [k, k], 'strides': list(strides), 'relu_input': relu,
         'hbm_floor_us': (x.numel() + cot.numel()) * 4 / 8e6}
  routes = {'fused': lambda: nn.conv2d(x, kernel, bias, strides, relu_input=relu), 'conv2d': lambda: conv2d_route(x, kernel, bias, strides, relu)}
  with torch.no_grad():
    row['max_abs_difference_conv2d'] = float((routes['fused']() - routes['conv2d']()).abs().max())
  for route, fn in routes.items():
    row['us_forward_' + route] = timed(no_grad(fn), steps)
    row['us_forward_backward_' + route] = timed(lambda fn=fn: torch.autograd.grad(fn(), leaves, cot), max(steps // 2, 1))
  fixed = (kernel.detach(), bias.detach())               # no weight gradient: forward and the adjoint alone
  row['us_forward_backward_in_x_fused'] = timed(lambda: torch.autograd.grad(nn.conv2d(x, *fixed, strides, relu_input=relu), [x], cot), max(steps // 2, 1))
  result['convolutions'][name] = row
  print(json.dumps({name: row}), flush=True)
  del x, kernel, bias, cot

# ---- 1 x 1 at stride 1: the kernel or torch.matmul -----------------------------------------------------------------------------------
for name, shape, ch_out in (('128_to_32', (BATCH, FRAMES, 58, 128), 32), ('32_to_128', (BATCH, FRAMES, 58, 32), 128),
                            ('256_to_1024', (BATCH, FRAMES, 8, 256), 1024)):
  x, kernel, bias, cot = operands(shape, ch_out, 1, 1, (1, 1))
  leaves = [x, kernel, bias]
  row = {'x': list(shape), 'ch_out': ch_out, 'hbm_floor_us': (x.numel() + cot.numel()) * 4 / 8e6}
  routes = {'fused': lambda: nn.conv2d(x, kernel, bias, (1, 1), relu_input=True),
            'matmul': lambda: torch.matmul(F.relu(x), kernel[0, 0]) + bias}
  for route, fn in routes.items():
    row['us_forward_' + route] = timed(no_grad(fn), 20)
    row['us_forward_backward_' + route] = timed(lambda fn=fn: torch.autograd.grad(fn(), leaves, cot), 10)
  result['one_by_one'][name] = row
  print(json.dumps({name: row}), flush=True)
  del x, kernel, bias, cot

# ---- the parts of one residual layer without shortcut at [32, 125, 58, 128] (ch = 32) ---------------------------------------------------
layer = nn.ResidualLayer(32, 1, False, 'layer', False, False)
x = torch.randn(BATCH, FRAMES, 58, 128, device=DEV, requires_grad=True)
cot = torch.randn(BATCH, FRAMES, 58, 128, device=DEV)
with torch.no_grad():
  layer(x)                                               # builds
mid = torch.randn(BATCH, FRAMES, 58, 32, device=DEV, requires_grad=True)
b0, b1, b2 = layer.bottleneck
mid_cot = torch.randn_like(mid)
parts = {'norm_input': (lambda: layer.norm_input(x), x, cot), 'conv_1x1_in': (lambda: b0(x, relu_input=True), x, mid_cot),
         'norm_1': (lambda: b1.norm(mid), mid, mid_cot), 'conv_3x3': (lambda: b1.conv(mid, relu_input=True), mid, mid_cot),
         'norm_2': (lambda: b2.norm(mid), mid, mid_cot), 'conv_1x1_out': (lambda: b2.conv(mid, relu_input=True, addend=x), mid, cot)}
row = {'x': list(x.shape), 'ch': 32, 'norm_type': 'layer'}
for direction in ('forward', 'forward_backward'):
  for name, (fn, leaf, part_cot) in parts.items():
    run = no_grad(fn) if direction == 'forward' else (lambda fn=fn, leaf=leaf, part_cot=part_cot: torch.autograd.grad(fn(), [leaf], part_cot))
    row['us_%s_%s' % (direction, name)] = timed(run, 10)
  whole = no_grad(lambda: layer(x)) if direction == 'forward' else (lambda: torch.autograd.grad(layer(x), [x] + list(layer.parameters()), cot))
  row['us_%s_layer' % direction] = timed(whole, 10)
  outside = sum(row['us_%s_%s' % (direction, name)][0] for name in parts if name.startswith('norm'))
  inside = sum(row['us_%s_%s' % (direction, name)][0] for name in parts if name.startswith('conv'))
  row['share_outside_conv_' + direction] = outside / (outside + inside)
result['residual_layer_parts'] = row
print(json.dumps(row), flush=True)
del x, cot, mid, layer, parts

# ---- ResNet('small') ----------------------------------------------------------------------------------------------------------------
net = nn.ResNet('small')
mag = torch.randn(BATCH, FRAMES, BINS, 1, device=DEV)
with torch.no_grad():
  out = net(mag)                                         # builds
params = list(net.parameters())
ocot = torch.randn_like(out)
framework = framework_resnet(net)
row = {'x': list(mag.shape), 'y': list(out.shape), 'convolutions': sum(1 for m in net.modules() if isinstance(m, nn.SpatialConv2D))}
with torch.no_grad():
  row['max_abs_difference_conv2d'] = float((net(mag) - framework(mag)).abs().max())
  row['max_abs_y'] = float(out.abs().max())
for route, fn in (('fused', lambda: net(mag)), ('conv2d', lambda: framework(mag))):
  row['us_forward_' + route] = timed(no_grad(fn), 2)
  row['us_forward_backward_' + route] = timed(lambda fn=fn: torch.autograd.grad(fn(), params, ocot), 2)
result['resnet_small'] = row
print(json.dumps(row), flush=True)

if len(sys.argv) > 1:
  with open(sys.argv[1], 'w') as fh:
    fh.write(json.dumps(result, indent=1) + '\n')
print(json.dumps(result))
