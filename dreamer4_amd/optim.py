"""MuonAdamAtan2: the optimiser the reference trains both whole models with (trainers.py:426, :833).

Muon (momentum, Nesterov, five Newton-Schulz iterations, scaled update, decoupled weight decay) on the 2-D trunk weights a model names with
`muon_parameters()`, Adam-atan2 on everything else.  Both groups step on the kernels of csrc/muon.hip: the whole Muon group in
passes * (2 + 3 * muon_steps) launches whatever the depth, the Adam-atan2 group and the gradient norm as multi-tensor kernels.
`muon_products='bf16'` (opt-in) takes the Newton-Schulz products from csrc/muon_bf16.hip, one more launch per pass.

`adam_atan2_pytorch` is third-party and absent here, so the contract is the arithmetic written in the class docstring, pinned in float64 by
tests/muon_ref.py.  Two things differ between published Muon variants and are constructor arguments: the momentum form (`muon_nesterov`) and the
scale on the orthogonalised update (`muon_update_scale`)."""
from __future__ import annotations

import ctypes as C
import math

import torch

from dreamer4_amd import _lib

UPDATE_SCALES = ('spectral', 'match_rms_adam', 'none')
PRODUCTS = {'fp32': 0, 'bf16': 1}             # muon_products -> the plan's `products` (d4_muon_plan_create_products)


def update_scale(kind, rows, cols):
    if kind == 'spectral':
        return math.sqrt(max(1., rows / cols))
    if kind == 'match_rms_adam':
        return 0.2 * math.sqrt(max(rows, cols))
    return 1.


def mark_mutated(tensors):
    """Tell autograd's version counters that `tensors` were written.  The kernels of this package write parameters through raw pointers, which no
    counter sees; the engines of DynamicsWorldModel and VideoTokenizer decide from `Tensor._version` when to rebuild the images they keep of the
    trunk weights, and autograd itself uses it to refuse a backward over a tensor saved before the write.  Host only: no launch,
    no synchronisation; views share their base's counter."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def newton_schulz(matrices, steps=5, coefs=(3.4445, -4.7750, 2.0315), eps=1e-7, workspace_bytes=256 << 20, products='fp32'):
    """The Newton-Schulz iteration of the Muon step alone (d4_newton_schulz: the optimiser's own launchers) on a list of 2-D fp32 HIP tensors:
    X = u / max(|u|_F, eps) oriented rows <= cols, `steps` times A = X X^T, B = b A + c A A, X <- a X + B X.  -> (outputs, passes).
    products='bf16': the products on the bf16 matrix pipe, under the contract of MuonAdamAtan2's `muon_products`."""
    if products not in PRODUCTS:
        raise ValueError(f'products must be one of {tuple(PRODUCTS)}, not {products!r}')
    lib = _lib.load()
    matrices = list(matrices)
    for u in matrices:
        if not u.is_cuda:
            raise _lib.D4Error('newton_schulz runs only on an MI355X (HIP) device: there is no CPU fallback')
        if u.ndim != 2 or u.dtype != torch.float32 or not u.is_contiguous():
            raise _lib.D4Error('newton_schulz takes contiguous 2-D fp32 tensors')
    device = matrices[0].device
    rows = (C.c_int32 * len(matrices))(*[u.shape[0] for u in matrices])
    cols = (C.c_int32 * len(matrices))(*[u.shape[1] for u in matrices])
    plan = C.c_void_p()
    _lib.check(lib.d4_muon_plan_create_products(len(matrices), rows, cols, int(workspace_bytes), PRODUCTS[products], C.byref(plan)))
    try:
        with torch.cuda.device(device):
            ws = torch.empty(lib.d4_muon_plan_workspace_bytes(plan), dtype=torch.uint8, device=device)
            out = [torch.empty_like(u) for u in matrices]
            a, b, c = coefs
            _lib.check(lib.d4_newton_schulz(plan, _ptr_array([u.data_ptr() for u in matrices]), _ptr_array([o.data_ptr() for o in out]),
                                            C.c_void_p(ws.data_ptr()), ws.numel(), int(steps), a, b, c, eps,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            passes = lib.d4_muon_plan_passes(plan)
            torch.cuda.current_stream().synchronize()       # the plan's device tables die with it
    finally:
        lib.d4_muon_plan_destroy(plan)
    return out, passes


class _Table:
    """A multi-tensor device table (d4_sumsq_multi / d4_adam_atan2_multi): re-uploaded only when a pointer or a size changed."""

    def __init__(self):
        self.key, self.buf, self.numel = None, None, None

    def bind(self, lib, key, numel, device):
        """-> (numel array, table tensor, upload flag)"""
        if key == self.key:
            return self.numel, self.buf, 0
        self.numel = (C.c_int64 * len(numel))(*numel)
        need = lib.d4_multi_table_bytes(len(numel), self.numel)
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            self.buf = torch.empty(need, dtype=torch.uint8, device=device)
        self.key = key
        return self.numel, self.buf, 1


class MuonAdamAtan2(torch.optim.Optimizer):
    """MuonAdamAtan2(muon_params, params, lr=1e-4, muon_lr=None, betas=(0.9, 0.99), weight_decay=0., a=1.27, b=1., muon_beta=0.95, muon_steps=5,
    muon_coefs=(3.4445, -4.7750, 2.0315), muon_eps=1e-7, muon_nesterov=True, muon_update_scale='spectral', remove_muon_params_from_params=True,
    *, max_grad_norm=None, workspace_bytes=256 << 20, muon_products='fp32')

    Muon group: every tensor of `muon_params` (2-D).  Per W [r][c] with gradient g:
        m <- lerp(m, g, 1 - muon_beta);  u = lerp(g, m, muon_beta) if muon_nesterov else m;  transposed if r > c;
        X = u / max(|u|_F, muon_eps);  muon_steps times: A = X X^T, B = b A + c A A, X <- a X + B X  with (a, b, c) = muon_coefs;  transposed back;
        s = sqrt(max(1, r / c)) ('spectral') | 0.2 sqrt(max(r, c)) ('match_rms_adam') | 1 ('none');
        W <- W (1 - lr_m weight_decay) - lr_m s X,  lr_m = muon_lr or lr.
    Adam-atan2 group: every tensor of `params` not in `muon_params` (by identity; with remove_muon_params_from_params=False a tensor in both
    lists raises ValueError).  With t counting this tensor's steps from 1:
        m <- lerp(m, g, 1 - beta1);  v <- lerp(v, g^2, 1 - beta2);
        W <- W (1 - lr weight_decay) - lr a atan2(m / (1 - beta1^t), b sqrt(v / (1 - beta2^t))).
    `max_grad_norm` (not a reference argument; both reference trainers call clip_grad_norm_ before every step): the global L2 norm of all
    gradients of both groups is reduced on the device in fixed order, with no host synchronisation, and g min(1, max_grad_norm / (norm + 1e-6))
    stands wherever g appears above; `.grad` itself is left untouched.
    `workspace_bytes` bounds the work buffers of one Muon pass (X, X', A, B per matrix): a group that needs more runs in several passes, with the
    same bits; one matrix that does not fit alone is an error that names it.
    `muon_products='bf16'` (opt-in; anything but 'fp32' / 'bf16' raises ValueError) runs the Newton-Schulz products on the bf16 matrix pipe
    (csrc/muon_bf16.hip).  Per matrix, oriented rows <= cols:
        m, u and the strip partials of sum u^2 are the unchanged fp32 arithmetic: `exp_avg` holds the same bits in both modes;
        X0 = bf16(u * 1 / max(|u|_F, muon_eps)): scaled in fp32 with the scale formed as above, rounded once (nearest even) after normalising,
             in one extra launch per pass;
        muon_steps times  A = bf16(X X^T),  B = bf16(b A + c (A A)),  X <- bf16(a X + B X):  every product takes bf16 operands with fp32
             accumulation in a fixed k order, its alpha E + beta acc epilogue is fp32 on the widened bf16 E and is rounded once on the store;
        every work buffer is bf16 (the workspace is not larger than the fp32 form's); X X^T is symmetric bit for bit, so the two symmetric
             stages still compute upper tiles only, and A A is computed as A A^T;
        finish reads the bf16 X and does the unchanged fp32 update of W.
    Equal inputs and state give equal bits, whatever the pass partition.  The mode is an attribute like `max_grad_norm`, not in `param_groups`:
    a state_dict written in one mode loads in the other (the state is the same fp32 `exp_avg`).

    Parameters whose `.grad` is None are skipped.  fp32, contiguous, HIP device only: CPU tensors raise D4Error (no CPU fallback).  State per
    parameter: `exp_avg`, `exp_avg_sq` (Adam-atan2 group) and `step`; state_dict() / load_state_dict() are torch.optim.Optimizer's own.
    The step is eager only: the bias corrections are host scalars and the pointer tables are rebuilt on the host when a `data_ptr` changed
    (zero_grad(set_to_none=True) reallocates gradients), so the step is NOT graph-capturable."""

    def __init__(self, muon_params, params, lr=1e-4, muon_lr=None, betas=(0.9, 0.99), weight_decay=0., a=1.27, b=1., muon_beta=0.95, muon_steps=5,
                 muon_coefs=(3.4445, -4.7750, 2.0315), muon_eps=1e-7, muon_nesterov=True, muon_update_scale='spectral',
                 remove_muon_params_from_params=True, *, max_grad_norm=None, workspace_bytes=256 << 20, muon_products='fp32'):
        if muon_update_scale not in UPDATE_SCALES:
            raise ValueError(f'muon_update_scale must be one of {UPDATE_SCALES}, not {muon_update_scale!r}')
        if not lr > 0. or (muon_lr is not None and not muon_lr > 0.):
            raise ValueError('lr and muon_lr must be positive')
        if not all(0. <= x < 1. for x in (*betas, muon_beta)):
            raise ValueError('betas and muon_beta must lie in [0, 1)')
        if not (isinstance(muon_steps, int) and 1 <= muon_steps <= 64):
            raise ValueError('muon_steps must be an integer in 1 .. 64')
        if len(muon_coefs) != 3:
            raise ValueError('muon_coefs is the triple (a, b, c) of the Newton-Schulz polynomial')
        if muon_products not in PRODUCTS:
            raise ValueError(f'muon_products must be one of {tuple(PRODUCTS)}, not {muon_products!r}')
        if max_grad_norm is not None and not max_grad_norm > 0.:
            raise ValueError('max_grad_norm must be positive (None: no clipping)')
        muon_params, params = list(muon_params), list(params)
        for i, p in enumerate(muon_params):
            if p.ndim != 2:
                raise ValueError(f'muon_params[{i}] has shape {tuple(p.shape)}: Muon takes 2-D tensors only')
        muon_ids = {id(p) for p in muon_params}
        if remove_muon_params_from_params:
            params = [p for p in params if id(p) not in muon_ids]
        elif any(id(p) in muon_ids for p in params):
            raise ValueError('a tensor is in both muon_params and params (remove_muon_params_from_params=False): it would be stepped twice')
        defaults = dict(lr=lr, muon_lr=muon_lr, betas=tuple(betas), weight_decay=weight_decay, a=a, b=b, muon_beta=muon_beta, muon_steps=muon_steps,
                        muon_coefs=tuple(muon_coefs), muon_eps=muon_eps, muon_nesterov=bool(muon_nesterov), muon_update_scale=muon_update_scale,
                        use_muon=False)
        groups = []
        if muon_params:
            groups.append(dict(params=muon_params, use_muon=True))
        if params:
            groups.append(dict(params=params, use_muon=False))
        super().__init__(groups, defaults)
        self.max_grad_norm = max_grad_norm
        self.workspace_bytes = int(workspace_bytes)
        self.muon_products = muon_products
        self._plans = {}                    # (device, shapes) -> (plan handle, workspace tensor)
        self._norm_table = _Table()
        self._adam_tables = {}              # (group index, step) order slot -> _Table
        self._norm = None
        self.last_launches = 0              # kernel launches of the last step() (tools/muon_step.py)

    def __del__(self):
        try:
            lib = _lib.load()
            for plan, _ in self._plans.values():
                lib.d4_muon_plan_destroy(plan)
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _usable(p):
        if not p.is_cuda:
            raise _lib.D4Error('MuonAdamAtan2 steps only on an MI355X (HIP) device: there is no CPU fallback')
        if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
            raise _lib.D4Error('MuonAdamAtan2 is fp32 only')
        if not p.is_contiguous():
            raise _lib.D4Error('MuonAdamAtan2 needs contiguous parameters')
        if p.grad.is_sparse:
            raise _lib.D4Error('MuonAdamAtan2 does not take sparse gradients')

    def _plan(self, lib, device, shapes):
        key = (device, shapes)
        hit = self._plans.get(key)
        if hit is None:
            rows = (C.c_int32 * len(shapes))(*[s[0] for s in shapes])
            cols = (C.c_int32 * len(shapes))(*[s[1] for s in shapes])
            plan = C.c_void_p()
            _lib.check(lib.d4_muon_plan_create_products(len(shapes), rows, cols, self.workspace_bytes, PRODUCTS[self.muon_products], C.byref(plan)))
            ws = torch.empty(lib.d4_muon_plan_workspace_bytes(plan), dtype=torch.uint8, device=device)
            hit = self._plans[key] = (plan, ws)
        return hit

    def muon_workspace_bytes(self):
        """bytes of the Muon workspaces allocated so far (one per distinct active set)"""
        return sum(ws.numel() for _, ws in self._plans.values())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        active = [[p for p in g['params'] if p.grad is not None and p.numel() > 0] for g in self.param_groups]
        flat = [p for ps in active for p in ps]
        if not flat:
            return loss
        for p in flat:
            self._usable(p)
        lib = _lib.load()
        device = flat[0].device
        if any(p.device != device for p in flat):
            raise _lib.D4Error('MuonAdamAtan2: all parameters must live on one device')
        launches = 0
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in flat]
            gof = {id(p): g for p, g in zip(flat, grads)}
            norm, max_norm = None, 0.
            if self.max_grad_norm is not None:
                if self._norm is None or self._norm.device != device:
                    self._norm = torch.zeros(1, device=device)
                gp = [g.data_ptr() for g in grads]
                numel, table, upload = self._norm_table.bind(lib, (device, tuple(gp), tuple(g.numel() for g in grads)), [g.numel() for g in grads], device)
                _lib.check(lib.d4_sumsq_multi(len(gp), numel, _ptr_array(gp), C.c_void_p(table.data_ptr()), table.numel(), upload,
                                              C.c_void_p(self._norm.data_ptr()), stream))
                norm, max_norm = C.c_void_p(self._norm.data_ptr()), float(self.max_grad_norm)
                launches += 2
            for gi, (group, ps) in enumerate(zip(self.param_groups, active)):
                if not ps:
                    continue
                for p in ps:
                    st = self.state[p]
                    if 'step' not in st:
                        st['step'] = 0
                        st['exp_avg'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        if not group['use_muon']:
                            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st['step'] = int(st['step']) + 1
                if group['use_muon']:
                    shapes = tuple((p.shape[0], p.shape[1]) for p in ps)
                    plan, ws = self._plan(lib, device, shapes)
                    lr = group['muon_lr'] if group['muon_lr'] is not None else group['lr']
                    ca, cb, cc = group['muon_coefs']
                    scales = (C.c_float * len(ps))(*[update_scale(group['muon_update_scale'], *s) for s in shapes])
                    _lib.check(lib.d4_muon_step(plan, _ptr_array([p.data_ptr() for p in ps]), _ptr_array([gof[id(p)].data_ptr() for p in ps]),
                                                _ptr_array([self.state[p]['exp_avg'].data_ptr() for p in ps]), scales, C.c_void_p(ws.data_ptr()), ws.numel(),
                                                lr, group['weight_decay'], group['muon_beta'], int(group['muon_nesterov']), group['muon_steps'],
                                                ca, cb, cc, group['muon_eps'], norm, max_norm, stream))
                    launches += lib.d4_muon_plan_passes(plan) * (2 + lib.d4_muon_plan_products(plan) + 3 * group['muon_steps'])     # bf16: + normalise
                    continue
                by_step = {}
                for p in ps:
                    by_step.setdefault(self.state[p]['step'], []).append(p)
                for slot, (t, tp) in enumerate(sorted(by_step.items())):
                    ptrs = [[p.data_ptr() for p in tp], [gof[id(p)].data_ptr() for p in tp], [self.state[p]['exp_avg'].data_ptr() for p in tp],
                            [self.state[p]['exp_avg_sq'].data_ptr() for p in tp]]
                    sizes = [p.numel() for p in tp]
                    tab = self._adam_tables.setdefault((gi, slot), _Table())
                    numel, table, upload = tab.bind(lib, (device, tuple(map(tuple, ptrs)), tuple(sizes)), sizes, device)
                    b1, b2 = group['betas']
                    _lib.check(lib.d4_adam_atan2_multi(len(tp), numel, *[_ptr_array(x) for x in ptrs], C.c_void_p(table.data_ptr()), table.numel(), upload, t,
                                                       group['lr'], b1, b2, group['weight_decay'], group['a'], group['b'], norm, max_norm, stream))
                    launches += 1
        mark_mutated(flat)
        self.last_launches = launches
        return loss
