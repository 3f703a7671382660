"""The bf16 training arithmetic against the fp32 path, one process, one box.   python tools/train_bf16_step.py [--skip-cfg5 | --cfg5-only]

  1. the workload of bench.py::train_flow_step (config 2's architecture, B = 16 x T = 16 frames of 15 tokens), flow-only and with the shortcut
     passes, `train_matmul_dtype` 'fp32' and 'bf16': median ms per step after warm-up; the fp32 figures are the ones to hold against
     `train_flow_step.flow_only_ms_per_step` / `with_shortcut_ms_per_step` of a `bench.py --full` line from the same box;
  2. the same at config 5's architecture (dim 1024, depth 12, 64 x 32 latents, 6 continuous actions), B = 4 x T = 16;
  3. the weight-gradient kernel alone (d4_gemm_tn_bf16) on the weight-gradient shapes of both sizes against d4_gemm_tn (fp32) on the same
     shapes, in TFLOP/s, beside the bf16 MFMA stream this box sustains (d4_measure_peaks).
Its output is kept as profiles/train_bf16_step.txt."""
import ctypes as C
import statistics
import sys
import time

sys.path.insert(0, __file__.rsplit('/', 2)[0])
import torch

from dreamer4_amd import DynamicsWorldModel, _lib
from dreamer4_amd.synthetic import randomize_weights

CFG2 = dict(dim=512, dim_latent=32, num_latent_tokens=32, depth=6, attn_heads=8, attn_dim_head=64,
            num_spatial_tokens=4, num_register_tokens=8, max_steps=64, multi_token_pred_len=8, num_discrete_actions=4)
CFG5 = dict(dim=1024, dim_latent=32, num_latent_tokens=64, depth=12, num_continuous_actions=6)
dev = torch.device('cuda:0')
lib = _lib.load()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def step_ms(m, lat, kw, prob, g, warm=3, reps=7):
    ts = []
    for i in range(warm + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for p in m.parameters():
            p.grad = None
        m(latents=lat, generator=g, prob_shortcut_train=prob, **kw).backward()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    # bench.py::train_flow_step's own method (4 steps back to back between two synchronisations, the second of two repetitions): the fp32
    # figure of config 2 is the one to hold against `train_flow_step.*_ms_per_step` of a `bench.py --full` line from the same box
    for rep in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(4):
            for p in m.parameters():
                p.grad = None
            m(latents=lat, generator=g, prob_shortcut_train=prob, **kw).backward()
        torch.cuda.synchronize(); b2b = 1e3 * (time.perf_counter() - t0) / 4
    return statistics.median(ts), min(ts), max(ts), b2b


def model_steps(name, cfg, B, T, discrete):
    g = torch.Generator(device=dev).manual_seed(1)
    lat = torch.randn(B, T, cfg['num_latent_tokens'], cfg['dim_latent'], device=dev, generator=g).clamp(-2, 2)
    kw = dict(discrete_actions=torch.randint(0, 4, (B, T, 1), device=dev, generator=g)) if discrete else \
        dict(continuous_actions=torch.rand(B, T, 6, device=dev, generator=g).clamp(0.05, 0.95))
    res = {}
    for arith in ('fp32', 'bf16'):
        torch.manual_seed(0)
        m = randomize_weights(DynamicsWorldModel(**cfg, train_matmul_dtype=arith)).to(dev)
        for label, prob in (('flow_only', 0.), ('with_shortcut', 1.)):
            res[arith, label] = step_ms(m, lat, kw, prob, g)
        del m
        torch.cuda.empty_cache()
    print(f'{name}: B = {B} x T = {T} frames, training forward + backward, ms per step: median (min .. max) of 7 after 3 warm-up steps')
    for label in ('flow_only', 'with_shortcut'):
        f, b = res['fp32', label], res['bf16', label]
        print(f'  {label:14s} fp32 {f[0]:8.2f} ({f[1]:.2f} .. {f[2]:.2f})   bf16 {b[0]:8.2f} ({b[1]:.2f} .. {b[2]:.2f})   fp32 / bf16 = {f[0] / b[0]:.2f}'
              f'   | 4 steps back to back (bench.py\'s method): fp32 {f[3]:.2f}  bf16 {b[3]:.2f}')
    sys.stdout.flush()
    return res


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def kernels(peak_bf16):
    part = torch.empty(8 << 20, device=dev)
    print(f'weight-gradient kernel alone: d4_gemm_tn_bf16 (bf16 images in, conversion not counted) vs d4_gemm_tn (fp32), slices by each kernel\'s shape rule; '
          f'bf16 MFMA stream of this box {peak_bf16:.0f} TF/s')
    print('     M      N      k     gemm_tn us   TF/s    gemm_tn_bf16 us   TF/s   speed-up   frac of bf16 stream')
    shapes = [(512, 512, 3840), (1536, 512, 3840), (2752, 512, 3840), (512, 1376, 3840),                         # config 2: to_out / q|k|v / proj_in / proj_out at 3840 rows
              (1024, 1024, 4864), (3072, 1024, 4864), (5472, 1024, 4864), (1024, 2736, 4864)]                    # config 5 at B x T = 4 x 16 (76 tokens per frame)
    for M, N, K in shapes:
        A = torch.randn(K, M, device=dev); B = torch.randn(K, N, device=dev)
        Ab, Bb = A.to(torch.bfloat16).contiguous(), B.to(torch.bfloat16).contiguous()
        Cf, Cb = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        f32 = lambda: _lib.check(lib.d4_gemm_tn(_lib.ptr(A), M, _lib.ptr(B), N, _lib.ptr(Cf), N, M, N, K, _lib.ptr(part), part.numel(), 0, 0, st))
        b16 = lambda: _lib.check(lib.d4_gemm_tn_bf16(_lib.ptr(Ab), M, _lib.ptr(Bb), N, _lib.ptr(Cb), N, M, N, K, _lib.ptr(part), part.numel(), 0, st))
        uf, ub = timeit(f32), timeit(b16)
        fl = 2. * M * N * K
        ref = Ab.double().t() @ Bb.double()
        err = ((Cb.double() - ref).abs().max() / ref.abs().max()).item()
        assert err < 1e-4, (M, N, K, err)
        print(f'  {M:5d}  {N:5d}  {K:5d}   {uf:10.1f}  {fl / uf / 1e6:6.1f}   {ub:14.1f}  {fl / ub / 1e6:6.1f}   {uf / ub:7.2f}   {fl / ub / 1e6 / peak_bf16:8.3f}')
    sys.stdout.flush()


def main():
    buf = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    hbm, f32, b16 = C.c_double(), C.c_double(), C.c_double()
    _lib.check(lib.d4_measure_peaks(_lib.ptr(buf), buf.numel(), C.byref(hbm), C.byref(f32), C.byref(b16), st))
    del buf
    torch.cuda.empty_cache()
    print(f'measured peaks of this box: stream copy {hbm.value:.0f} GB/s, f32 MFMA stream {f32.value:.1f} TF/s, bf16 MFMA stream {b16.value:.1f} TF/s')
    if '--cfg5-only' not in sys.argv:
        kernels(b16.value)
        model_steps('config 2 architecture (bench.py train_flow_step)', CFG2, 16, 16, True)
    if '--skip-cfg5' not in sys.argv:
        model_steps('config 5 architecture', CFG5, 4, 16, False)


if __name__ == '__main__':
    main()
