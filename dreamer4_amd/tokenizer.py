"""Host-side mirror of the reference `VideoTokenizer` for its two inference paths:
`decode(latents)` — what `DynamicsWorldModel.generate(return_decoded_video=True)` calls (dreamer4/dreamer4.py:4186-4237, 6694-6711) —
and `tokenize(video)` — what `generate(prompt=video)` and `DynamicsWorldModel.forward(video=...)` call (dreamer4.py:4107-4113,
6376-6387).

Same constructor keyword names as the reference (dreamer4.py:3686-3764), the same state_dict key names for the parameters
(`latents_to_decoder.*`, `time_embed.*`, `noised_patch_to_tokens.*`, `decoder.*`; `patch_to_tokens.*`, `latent_tokens`,
`encoder_transformer.*`, `encoded_to_latents.*`), so a reference tokenizer checkpoint loads with `load_state_dict`.  The compute is
the HIP engine in decoder / encoder mode (include/d4hip.h `d4_decoder_forward`, `d4_encoder_forward`): the dynamics model's trunk
kernels over [patches | latent tokens] per frame, a wide attention kernel for the ~100-token space layers, patchify / un-patchify
kernels.  Supported subset = the reference defaults: flow decoder with `decoder_flow_steps` Euler steps, no slot attention, causal conv,
MOSS, aug conditioning, PoPE, separate flow decoder, BYOL.

`forward(video_or_image, ...)` is the training forward (dreamer4.py:4239-4603) for the same subset: MAE masking, encoder, tanh bottleneck,
one flow-decoder step at a drawn time, the v-space or x-space reconstruction loss with the reference's loss normalisation, autograd to
every parameter the loss reaches.  It runs `trunk_ops.tokenizer_losses`: both trunks on the differentiable HIP blocks, the passes over
pixels on the operators of csrc/tok_train.hip.  Three latent regularisers are optional terms of it, each behind the reference's
weight argument (default 0.: nothing changes): SIGReg of the latents before the tanh, the orthogonality loss of a frame's latent tokens (both fused
forward + backward operators of csrc/tok_reg.hip) and the latent consistency loss, a second encoder pass on the decoder's output with the encoder
frozen.  LPIPS (no VGG weights), the decorrelation and latent-autoregression losses, `time_lens`, time caches, aug conditioning
and BYOL are outside the subset and raise."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch
from torch import nn

from dreamer4_amd import _lib
from dreamer4_amd.checkpoint import SaveLoad
from dreamer4_amd.trunk_ops import ENCODER_KEYS
from dreamer4_amd.world_model import MLP_RECIPES, _linear_b, _linear_w, _register, mlp_param_specs, mlp_widths, transformer_muon_parameters

TokenizerLosses = namedtuple('TokenizerLosses', ('recon', 'flow_recon', 'lpips', 'time_decorr', 'space_decorr', 'latent_ortho', 'latent_ar', 'latent_ar_sigreg',
                                                 'latent_consistency', 'latent_sigreg', 'h_net', 'byol'))       # dreamer4.py:118
VideoTokenizerIntermediates = namedtuple('VideoTokenizerIntermediates', ('losses', 'recon'))

_UNSUPPORTED = dict(
    latent_init_patch_size=None, encoder_full_spatial_attn=False, decoder_full_spatial_attn=False, attn_kwargs={}, ff_kwargs={},
    use_causal_conv3d=False, use_shifted_patch_tokenization=False, encoder_moss_layers=(), decoder_moss_layers=(), use_time_rnn=False,
    time_attention_use_pope=False, space_attention_use_pope=False, h_net_layer=None, slot_attention_initted_latents=False,
    decoder_slot_attention_initted_spatial_tokens=False, mot_temporal=False, has_aug_conditioning=False, separate_flow_decoder=False,
    encode_temporal_diff=False, has_byol=False, decoder_pos_emb_mlp_activation='silu', attn_softclamp_value=50.,
)


_NORMALIZER_KEY = 'recon_loss_normalizer.exp_avg_sq'
# the latent regularisers: TokenizerLosses field -> the reference's LossNormalizer buffer; the state exists only when the term's weight is > 0
_REG_NORMALIZER_KEYS = {f: f'{f}_loss_normalizer.exp_avg_sq' for f in ('latent_sigreg', 'latent_ortho', 'latent_consistency')}
_SIGREG_KWARGS = ('num_slices', 'domain', 'num_knots')


class VideoTokenizer(SaveLoad, nn.Module):
    def __init__(self, dim, dim_latent, patch_size, image_size=None, image_height=None, image_width=None, num_latent_tokens=64,
                 encoder_depth=4, decoder_depth=4, time_block_every=4, attn_dim_head=64, attn_heads=8, decoder_pos_mlp_depth=2,
                 channels=3, decoder_flow_steps=1, head_mlp_recipe='pre_rms', wide_frames=False, attn_products='fp32',
                 train_wide_frames=False, lpips_loss_weight=0.2, decoder_v_space_loss=True, matmul_dtype='fp32', latent_sigreg_loss_weight=0.,
                 latent_sigreg_loss_kwargs=dict(num_slices=256), latent_ortho_loss_weight=0., latent_consistency_loss_weight=0., **kwargs):
        """`wide_frames` is not a reference argument: False (default) the decoder and encoder engines take at most 160 tokens (patches +
        latents) and 64 latent tokens per frame; True up to 1024 of each, on the tiled attention core of csrc/attn_wide_mfma.hip above 64
        items per side, and encoder / decoder trunks of depth >= 32 (up to 1024 pooled layer hiddens, the chunked pool mix of
        csrc/pool_mix_deep.hip; refused without the option).
        `attn_products` is not a reference argument either: 'fp32' (default) the wide core's two products on the f32-input MFMA, as ever;
        'bf16' (needs `wide_frames=True`) on the bf16 MFMA with bf16-rounded q, k', v' and softmax numerators and fp32 accumulation
        (csrc/attn_wide_bf16.hip).  Attentions of at most 64 items per side keep their kernels and bits.
        `train_wide_frames` (not a reference argument, the meaning it has on DynamicsWorldModel): False (default) the training forward takes at
        most 64 tokens (patches + latents) per frame; True up to 1024, on the tiled training attention core.
        `matmul_dtype` is not a reference argument either: 'fp32' (default) every GEMM of `decode` and `tokenize` on the f32-input MFMA, as ever
        and bit for bit; 'bf16' the Linears inside the two trunks (fused q|k|v|gates|mix projection, attention output, both feedforward projections,
        the attention pools' key / value / output projections, the encoder's final special cross-attention and feedforward) on bf16-rounded operands
        with fp32 accumulation — the kernels of the bf16 dynamics engine.  Norms, attention cores (unless `attn_products='bf16'`), softmax, the
        residual stream, the Euler step and the four end projections (patch rows -> tokens and its LayerNorm, latents -> decoder tokens, tokens ->
        patch rows, latent tokens -> latents and the tanh) stay fp32.  Independent of `wide_frames`, `attn_products`,
        `train_wide_frames` and of a world model's own `matmul_dtype`.  The training `forward` stays fp32 whatever the option says.
        `lpips_loss_weight` and `decoder_v_space_loss` are the reference's; the first is only stored (any value constructs, `forward` needs 0.).
        `latent_sigreg_loss_weight`, `latent_sigreg_loss_kwargs` (keys num_slices, domain, num_knots: the arguments of the reference's sigreg),
        `latent_ortho_loss_weight` and `latent_consistency_loss_weight` are the reference's (dreamer4.py:3995-4052), with its defaults: a weight > 0 adds
        that term to the training forward and, under loss normalisation, its normaliser state; at 0 nothing changes."""
        latent_sigreg_loss_kwargs = dict(latent_sigreg_loss_kwargs or {})       # the recorded config holds its own copy, never the shared default
        config = dict(locals())
        super().__init__()
        self._record_config(config)
        for k, v in kwargs.items():
            if k in _UNSUPPORTED:
                if v != _UNSUPPORTED[k]:
                    raise NotImplementedError(f'{k}={v!r} is outside the supported decode subset (reference defaults only)')
            elif k not in ('lpips_loss_network', 'per_image_patch_mask_prob', 'use_loss_normalization'):
                raise NotImplementedError(f'{k!r}: outside the subset the tokenizer mirror implements')
        assert image_size is not None or (image_height is not None and image_width is not None), \
            'either image_size or both image_height and image_width must be provided'
        if decoder_flow_steps < 1:
            raise NotImplementedError('decoder_flow_steps = 0 (no flow decoder) is not implemented')
        if attn_dim_head != 64:
            raise NotImplementedError('the decoder engine needs attn_dim_head == 64')
        self.dim, self.dim_latent, self.patch_size, self.channels = dim, dim_latent, patch_size, channels
        self.image_height = image_height if image_height is not None else image_size
        self.image_width = image_width if image_width is not None else image_size
        self.num_latent_tokens, self.decoder_depth, self.time_block_every = num_latent_tokens, decoder_depth, time_block_every
        self.encoder_depth = encoder_depth
        self.attn_heads, self.attn_dim_head = attn_heads, attn_dim_head
        self.decoder_pos_mlp_depth, self.decoder_flow_steps = decoder_pos_mlp_depth, decoder_flow_steps
        self.head_mlp_recipe = head_mlp_recipe
        self.wide_frames = bool(wide_frames)
        self.train_wide_frames = bool(train_wide_frames)
        self.lpips_loss_weight, self.decoder_v_space_loss = float(lpips_loss_weight), bool(decoder_v_space_loss)
        self.use_loss_normalization = bool(kwargs.get('use_loss_normalization', True))
        self.per_image_patch_mask_prob = tuple(kwargs.get('per_image_patch_mask_prob', (0., 0.9)))
        self.latent_sigreg_loss_kwargs = dict(latent_sigreg_loss_kwargs)
        for k in self.latent_sigreg_loss_kwargs:
            if k not in _SIGREG_KWARGS:
                raise NotImplementedError(f'latent_sigreg_loss_kwargs[{k!r}]: the keys are {_SIGREG_KWARGS}')
        self.loss_weights = dict(latent_sigreg=float(latent_sigreg_loss_weight), latent_ortho=float(latent_ortho_loss_weight),
                                 latent_consistency=float(latent_consistency_loss_weight))
        self.latent_sigreg_loss_weight, self.latent_ortho_loss_weight = self.loss_weights['latent_sigreg'], self.loss_weights['latent_ortho']
        self.latent_consistency_loss_weight = self.loss_weights['latent_consistency']
        if attn_products not in ('fp32', 'bf16'):
            raise ValueError("attn_products must be 'fp32' or 'bf16'")
        if attn_products == 'bf16' and not self.wide_frames:
            raise ValueError("attn_products='bf16' needs wide_frames=True: only the wide attention core has a bf16 form")
        self.attn_products = attn_products
        if matmul_dtype not in ('fp32', 'bf16'):
            raise ValueError("matmul_dtype must be 'fp32' or 'bf16'")
        self.matmul_dtype = matmul_dtype
        self.latent_shape = (num_latent_tokens, dim_latent)
        self.ff_inner = int(dim * 4 * 2 / 3)
        self._build_parameters()
        self._engines = {}          # mode -> dict(engine, caps, ws, bound_sig, prep_version)

    def _build_parameters(self):
        D, dl, h, dh = self.dim, self.dim_latent, self.attn_heads, self.attn_dim_head
        hd, dp = h * dh, self.channels * self.patch_size ** 2
        reg = lambda k, t: _register(self, k, t)

        def attn(pre, heads, ctx_norm, mix, dh_=dh):
            inner = heads * dh_
            reg(pre + 'norm.weight', torch.ones(D))
            if ctx_norm:
                reg(pre + 'norm_context.weight', torch.ones(D))
            for nm, shape in (('to_q', (inner, D)), ('to_k', (inner, D)), ('to_v', (inner, D)), ('to_out', (D, inner))):
                reg(pre + nm + '.weight', _linear_w(*shape))
            reg(pre + 'to_gates.0.weight', _linear_w(heads, D))
            reg(pre + 'k_heads_rmsnorm.gamma', torch.zeros(heads, dh_))
            if mix:
                reg(pre + 'to_learned_value_residual_mix.0.weight', _linear_w(heads, D))
                reg(pre + 'to_learned_value_residual_mix.0.bias', _linear_b(heads, D))

        def ff(pre):
            reg(pre + 'norm.weight', torch.ones(D))
            reg(pre + 'proj_in.weight', _linear_w(2 * self.ff_inner, D)); reg(pre + 'proj_in.bias', _linear_b(2 * self.ff_inner, D))
            reg(pre + 'proj_out.weight', _linear_w(D, self.ff_inner)); reg(pre + 'proj_out.bias', _linear_b(D, self.ff_inner))

        reg('latents_to_decoder.weight', _linear_w(D, dl))
        reg('time_embed.weight', torch.randn(self.decoder_flow_steps, D))
        reg('noised_patch_to_tokens.1.weight', _linear_w(D, dp)); reg('noised_patch_to_tokens.1.bias', _linear_b(D, dp))
        reg('noised_patch_to_tokens.2.weight', torch.ones(D))
        fan_in = 2
        for key, shape, kind in mlp_param_specs(self.head_mlp_recipe, mlp_widths(2, 2 * D, D, self.decoder_pos_mlp_depth)):
            if kind == 'norm_w':
                reg('decoder.to_decoder_pos_emb.' + key, torch.ones(shape))
            elif kind == 'norm_b':
                reg('decoder.to_decoder_pos_emb.' + key, torch.zeros(shape))
            elif kind == 'lin_w':
                reg('decoder.to_decoder_pos_emb.' + key, _linear_w(*shape)); fan_in = shape[1]
            else:
                reg('decoder.to_decoder_pos_emb.' + key, _linear_b(shape[0], fan_in))
        reg('decoder.tokens_to_patch.0.weight', _linear_w(dp, D)); reg('decoder.tokens_to_patch.0.bias', _linear_b(dp, D))

        def trunk(tp, depth):
            inv_freq = 1.0 / (10000. ** (torch.arange(0, dh, 2).float() / dh))
            _register(self, tp + 'time_rotary.inv_freq', inv_freq, buffer=True)
            reg(tp + 'to_value_residual.0.weight', torch.ones(D)); reg(tp + 'to_value_residual.1.weight', _linear_w(hd, D))
            for i in range(depth):
                attn(f'{tp}layers.{i}.2.fn.', h, False, True)
                ff(f'{tp}layers.{i}.3.fn.')
            for i in range(depth - 1):
                attn(f'{tp}attn_pools.{i}.fn.attn.', 4, True, False, 64)
            attn(tp + 'final_attn_pool.fn.attn.', 4, True, False, 64)
            reg(tp + 'final_norm.weight', torch.ones(D))
            attn(tp + 'final_special_cross_attn.fn.', h, True, True)
            ff(tp + 'final_special_ff.fn.')

        # the decoder trunk's final special cross-attention / feedforward (dreamer4.py:2901-2907) update only the last latent token,
        # which the decoder never reads back: the parameters exist for key parity and are not bound to the decoder engine
        trunk('decoder.transformer.', self.decoder_depth)
        # encoder (dreamer4.py:3796, 3838-3848, 3912-3936)
        reg('latent_tokens', torch.randn(self.num_latent_tokens, D) * 1e-2)
        reg('mask_token', torch.randn(D) * 1e-2)             # training-only (MAE masking, dreamer4.py:4318-4340); key parity
        reg('patch_to_tokens.1.weight', _linear_w(D, dp)); reg('patch_to_tokens.1.bias', _linear_b(D, dp))
        reg('patch_to_tokens.2.weight', torch.ones(D))
        trunk('encoder_transformer.', self.encoder_depth)
        reg('encoded_to_latents.weight', _linear_w(dl, D))
        _register(self, 'zero', torch.tensor(0.), buffer=True, persistent=False)
        # LossNormalizer state of the training forward (dreamer4.py:629-669, 4037).  NOT persistent, unlike the reference's: the mirror's
        # state_dict stays the parameter set the inference paths load; load_state_dict still takes the key from a reference checkpoint
        if self.use_loss_normalization:
            _register(self, _NORMALIZER_KEY, torch.ones(1), buffer=True, persistent=False)
            for f, key in _REG_NORMALIZER_KEYS.items():
                if self.loss_weights[f] > 0.:
                    _register(self, key, torch.ones(1), buffer=True, persistent=False)

    def muon_parameters(self):
        """dreamer4.py:4096-4105: the encoder transformer's and the decoder transformer's Muon parameters (no separate flow decoder in the subset)."""
        return [*transformer_muon_parameters(self.encoder_transformer), *transformer_muon_parameters(self.decoder.transformer)]

    def load_state_dict(self, state_dict, strict=True, **kwargs):
        own = dict(self.named_buffers())
        for key in (_NORMALIZER_KEY, *_REG_NORMALIZER_KEYS.values()):
            if key in state_dict:
                state_dict = dict(state_dict)
                state = state_dict.pop(key)
                if key in own:                                         # a term this tokenizer does not train with: the reference's state is dropped
                    with torch.no_grad():
                        own[key].copy_(torch.as_tensor(state).reshape(1))
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    @property
    def device(self):
        return self.zero.device

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    _ENCODER_KEYS = ENCODER_KEYS

    def _engine_tensors(self, mode):
        out = {}
        for k, v in list(self.named_parameters()) + list(self.named_buffers()):
            if k in ('zero', 'mask_token', _NORMALIZER_KEY, *_REG_NORMALIZER_KEYS.values()):
                continue
            enc = k.startswith(self._ENCODER_KEYS)
            if mode == 2 and enc:
                out[k] = v
            elif mode == 1 and not enc and 'final_special' not in k:
                out[k] = v
        return out

    def __deepcopy__(self, memo):
        # engine handles are per-instance device state: a copy starts without any (DynamicsWorldModel deep-copies its tokenizer, dreamer4.py:4788)
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == '_engines' else copy.deepcopy(v, memo)
        return new

    def __del__(self):
        try:
            lib = _lib.load()
            for st in self._engines.values():
                if st['engine'] is not None:
                    lib.d4_engine_destroy(st['engine'])
            self._engines.clear()
        except Exception:
            pass

    def _make_config(self, mode, caps):
        """The engine configuration of `mode` (1 decoder, 2 encoder) sized for caps = (batch, frames).  Host only: no device is touched."""
        c = _lib.Config()
        c.mode = mode
        c.dim, c.dim_latent, c.num_latent_tokens = self.dim, self.dim_latent, self.num_latent_tokens
        c.depth = self.decoder_depth if mode == 1 else self.encoder_depth
        c.time_block_every, c.attn_heads, c.attn_dim_head, c.attn_softclamp_value = self.time_block_every, self.attn_heads, self.attn_dim_head, 50.
        c.num_spatial_tokens, c.num_register_tokens, c.max_steps, c.multi_token_pred_len = 0, 0, 64, 1
        c.reward_num_bins = c.value_num_bins = 3
        c.pool_heads, c.pool_dim_head = 4, 64
        c.head_mlp_recipe = MLP_RECIPES[self.head_mlp_recipe]
        c.patch_size, c.channels, c.image_height, c.image_width = self.patch_size, self.channels, self.image_height, self.image_width
        c.decoder_flow_steps, c.decoder_pos_mlp_depth = self.decoder_flow_steps, self.decoder_pos_mlp_depth
        c.max_batch, c.max_frames, c.max_parallel_frames, c.max_learn_rows = caps[0], caps[1], caps[1], 0
        c.wide_frames = 3 if self.attn_products == 'bf16' else int(self.wide_frames)
        c.matmul_bf16 = 1 if self.matmul_dtype == 'bf16' else 0
        return c

    def _ensure_engine(self, batch, frames, mode=1):
        if self.device.type != 'cuda':
            raise _lib.D4Error('VideoTokenizer runs only on an MI355X (HIP) device: there is no CPU fallback')
        lib = _lib.load()
        st = self._engines.setdefault(mode, dict(engine=None, caps=None, ws=None, bound_sig=None, prep_version=None))
        if st['caps'] is None or batch > st['caps'][0] or frames > st['caps'][1]:
            old = st['caps'] or (0, 0)
            caps = (max(batch, old[0]), max(frames, old[1]))
            if st['engine'] is not None:
                lib.d4_engine_destroy(st['engine'])
                st['engine'] = None
            c = self._make_config(mode, caps)
            eng = C.c_void_p()
            _lib.check(lib.d4_engine_create(C.byref(c), C.byref(eng)))
            st['engine'], st['caps'] = eng, caps
            nbytes = lib.d4_engine_workspace_bytes(eng)
            st['ws'] = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            base = st['ws'].data_ptr()
            _lib.check(lib.d4_engine_set_workspace(eng, C.c_void_p(base + (-base) % 256), nbytes))
            st['bound_sig'] = None
        tensors = self._engine_tensors(mode)
        sig = tuple((k, t.data_ptr()) for k, t in tensors.items())
        ver = tuple(t._version for t in tensors.values())
        if sig != st['bound_sig']:
            for k, t in tensors.items():
                assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device, k
                _lib.check(lib.d4_engine_bind(st['engine'], k.encode(), _lib.ptr(t), None, t.numel()))
            st['bound_sig'], st['prep_version'] = sig, None
        if ver != st['prep_version']:
            _lib.check(lib.d4_engine_prepare(st['engine'], self._stream()))
            st['prep_version'] = ver
        return st['engine']

    def invalidate_prepared(self):
        """Force both engines' weight images to be rebuilt on the next `decode` / `tokenize`.  Needed only after a write autograd's version
        counter cannot see (`p.data.copy_(...)`, `dist.broadcast(p.data)`, a third party's raw pointer).  Every call looks at the parameters
        the module holds then, so in-place updates, torch optimisers, MuonAdamAtan2 (it marks what it stepped as mutated), `load_state_dict`
        copying or with `assign=True` and replaced Parameter objects are detected with no call."""
        for st in self._engines.values():
            st['prep_version'] = None

    # ------------------------------------------------------------------------------------------ decode
    @torch.no_grad()
    def decode(self, latents, height=None, width=None, aug_id=None, return_recons_across_steps=False, *, noise=None, generator=None,
               max_batch=None):
        """VideoTokenizer.decode (dreamer4.py:4186-4237): latents (b, t, n, d) -> video (b, c, t, h, w).  `noise` injects the one
        random draw (the initial flow sample, dreamer4.py:4212) for parity runs; `max_batch` bounds the trajectories decoded per
        engine pass (workspace: ~0.1 MB per token row)."""
        if aug_id not in (None, 0, False):
            raise NotImplementedError('aug conditioning is not implemented')
        if (height not in (None, self.image_height)) or (width not in (None, self.image_width)):
            raise NotImplementedError('decoding at a resolution other than the one given to the constructor is not implemented')
        B, T = latents.shape[:2]
        dev = self.device
        lat = latents.to(dev).float().reshape(B, T, *self.latent_shape).contiguous()
        H, W, Cc = self.image_height, self.image_width, self.channels
        if noise is None:
            noise = torch.randn(B, Cc, T, H, W, device=dev, generator=generator)
        video = noise.to(dev).float().contiguous().clone()
        assert video.shape == (B, Cc, T, H, W)
        chunk = max_batch or B
        lib = _lib.load()
        steps = self.decoder_flow_steps
        preds = []
        for i in range(steps):
            pred = torch.empty_like(video)
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                eng = self._ensure_engine(b1 - b0, T)
                _lib.check(lib.d4_decoder_forward(eng, _lib.ptr(lat[b0:b1]), _lib.ptr(video[b0:b1]), i, b1 - b0, T, _lib.ptr(pred[b0:b1]), self._stream()))
            # video += (pred - video) / (1 - i / steps) * (1 / steps)          dreamer4.py:4226-4230
            _lib.check(lib.d4_euler_step(_lib.ptr(video), _lib.ptr(pred), video.numel(), 1. - i / steps, 1. / steps, self._stream()))
            if return_recons_across_steps:
                preds.append(pred)
        return (video, preds) if return_recons_across_steps else video

    # ------------------------------------------------------------------------------------------ tokenize
    @torch.no_grad()
    def tokenize(self, video, aug_id=None, *, max_batch=None):
        """VideoTokenizer.tokenize (dreamer4.py:4107-4113): video (b, c, t, h, w) or images (b, c, h, w) -> latents (b, t, n, d) in
        (-1, 1): eval-mode `forward(return_latents=True)` (dreamer4.py:4239-4433, no MAE masking).  `max_batch` bounds the clips
        encoded per engine pass."""
        if aug_id not in (None, 0, False):
            raise NotImplementedError('aug conditioning is not implemented')
        dev = self.device
        if video.ndim == 4:
            video = video.unsqueeze(2)                     # images: a one-frame video (dreamer4.py:4257-4258)
        assert video.ndim == 5, 'video must be (batch, channels, time, height, width)'
        B, Cc, T, H, W = video.shape
        assert Cc == self.channels, f'expected {self.channels} channels, got {Cc}'
        if (H, W) != (self.image_height, self.image_width):
            raise NotImplementedError('tokenizing at a resolution other than the one given to the constructor is not implemented')
        video = video.to(dev).float().contiguous()
        out = torch.empty(B, T, *self.latent_shape, device=dev)
        chunk = max_batch or B
        lib = _lib.load()
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            eng = self._ensure_engine(b1 - b0, T, mode=2)
            _lib.check(lib.d4_encoder_forward(eng, _lib.ptr(video[b0:b1]), b1 - b0, T, _lib.ptr(out[b0:b1]), self._stream()))
        return out

    # ------------------------------------------------------------------------------------------ training forward
    def _train_weights(self):
        return {**dict(self.named_parameters()), **{k: v for k, v in self.named_buffers() if k.endswith('inv_freq')}}

    def _is_time(self, depth):
        return [((i + 1) % self.time_block_every) == 0 for i in range(depth)]

    def _normalize_loss(self, loss, update_ema, beta=0.95, eps=1e-6, key=_NORMALIZER_KEY):
        """LossNormalizer.forward (dreamer4.py:645-669), the arithmetic of DynamicsWorldModel._normalize_loss, on the state buffer `key`."""
        if not self.use_loss_normalization:
            return loss
        buf = self.get_buffer(key)
        rms = buf.sqrt()
        if update_ema:
            with torch.no_grad():
                buf.lerp_(loss.detach().reshape(buf.shape).square(), 1. - beta)
        return loss / rms.clamp(min=eps).reshape(loss.shape)

    def forward(self, video_or_image, return_latents=False, mask_patches=None, patch_mask=None, return_intermediates=False, update_loss_ema=None,
                time_cache=None, return_time_cache=False, time_lens=None, aug_id=None, cfg_dropout_aug=None, byol_target_latents=None, *,
                draws=None, generator=None):
        """VideoTokenizer.forward (dreamer4.py:4239-4603) for the supported subset: video (b, c, t, h, w) or images (b, c, h, w) -> total loss, or
        (total, (TokenizerLosses, reconstruction)) with `return_intermediates`, or the latents (with gradient) with `return_latents`.
        `draws` = dict(patch_mask=, time_indices=, noise=, sigreg_projs=) injects the random draws (parity runs; a missing entry is drawn); otherwise
        they come from `generator` on the device.  `sigreg_projs` is the raw (num_slices, dim_latent) normal draw of the SIGReg term, read only when its
        weight is > 0 (the reference draws it a second time inside the consistency term's nested forward and discards that value: not imitated).  More than 64 tokens per frame need `train_wide_frames=True`.  The training forward is fp32:
        `matmul_dtype='bf16'` changes `decode` and `tokenize` only."""
        from dreamer4_amd import trunk_ops
        for name, val in (('time_lens', time_lens), ('time_cache', time_cache), ('byol_target_latents', byol_target_latents)):
            if val is not None:
                raise NotImplementedError(f'{name}= is outside the subset of the tokenizer training forward')
        if return_time_cache:
            raise NotImplementedError('return_time_cache= is outside the subset of the tokenizer training forward')
        if aug_id not in (None, 0, False):
            raise NotImplementedError('aug_id=: aug conditioning is not implemented')
        if not return_latents and self.lpips_loss_weight > 0.:
            raise NotImplementedError(f'lpips_loss_weight={self.lpips_loss_weight}: the LPIPS loss needs VGG weights this package does not carry; '
                                      'construct the tokenizer with lpips_loss_weight=0.')
        dev = self.device
        if dev.type != 'cuda' or video_or_image.device.type != 'cuda':
            raise _lib.D4Error('VideoTokenizer runs only on an MI355X (HIP) device: there is no CPU fallback')
        mask_patches = (self.training and not return_latents) if mask_patches is None else mask_patches
        is_image = video_or_image.ndim == 4
        video = video_or_image.unsqueeze(2) if is_image else video_or_image
        assert video.ndim == 5, 'video must be (batch, channels, time, height, width)'
        video = video.float().contiguous()
        B, Cc, T, H, W = video.shape
        assert Cc == self.channels, f'expected {self.channels} channels, got {Cc}'
        if (H, W) != (self.image_height, self.image_width):
            raise NotImplementedError('training at a resolution other than the one given to the constructor is not implemented')
        ps = self.patch_size
        nh, nw = H // ps, W // ps
        draws = dict(draws or {})
        if patch_mask is None:
            patch_mask = draws.get('patch_mask')
        if patch_mask is None and mask_patches:                                # dreamer4.py:4336-4342
            lo, hi = self.per_image_patch_mask_prob
            prob = torch.rand(B, T, device=dev, generator=generator) * (hi - lo) + lo
            patch_mask = torch.bernoulli(prob[:, :, None, None].expand(B, T, nh, nw), generator=generator) == 1.
        if patch_mask is not None:
            patch_mask = patch_mask.to(dev).bool()
            assert patch_mask.shape == (B, T, nh, nw), f'patch_mask must be {(B, T, nh, nw)}'
        Wt = self._train_weights()
        cfg = dict(patch_size=ps, num_latent_tokens=self.num_latent_tokens, encoder_is_time=self._is_time(self.encoder_depth), wide=self.train_wide_frames)
        if return_latents:
            return trunk_ops.tokenizer_latents(Wt, video, patch_mask=patch_mask, **cfg)
        time_indices, noise = draws.get('time_indices'), draws.get('noise')
        if time_indices is None:
            time_indices = torch.randint(0, self.decoder_flow_steps, (B,), device=dev, generator=generator)
        if noise is None:
            noise = torch.randn(video.shape, device=dev, generator=generator)
        noise = noise.to(dev).float().reshape(video.shape).contiguous()
        used = {f for f, w in self.loss_weights.items() if w > 0.}
        reg_kw, tdraws = {}, dict(patch_mask=patch_mask, time_indices=time_indices.to(dev).long(), noise=noise)
        if 'latent_sigreg' in used:
            sk = dict(self.latent_sigreg_loss_kwargs)
            shape = (int(sk.pop('num_slices', 1024)), self.dim_latent)          # sigreg's own default number of slices
            projs = draws.get('sigreg_projs')
            if projs is None:
                projs = torch.randn(shape, device=dev, generator=generator)
            tdraws['sigreg_projs'] = projs.to(dev).float().reshape(shape).contiguous()
            reg_kw['sigreg_kwargs'] = sk
        recon, latents, recon_video, regs = trunk_ops.tokenizer_losses(
            Wt, video, draws=tdraws, decoder_is_time=self._is_time(self.decoder_depth),
            decoder_flow_steps=self.decoder_flow_steps, decoder_pos_mlp_depth=self.decoder_pos_mlp_depth, head_mlp_recipe=self.head_mlp_recipe,
            v_space=self.decoder_v_space_loss, return_recon_video=return_intermediates, ortho='latent_ortho' in used,
            consistency='latent_consistency' in used, **reg_kw, **cfg)
        update = self.training if update_loss_ema is None else update_loss_ema
        recon = self._normalize_loss(recon, update)
        total = recon                                                          # the terms of dreamer4.py:4576-4589 the subset has, in its order
        terms = dict(latent_ortho=regs['ortho'], latent_consistency=regs['consistency'], latent_sigreg=regs['sigreg'])
        for f in ('latent_ortho', 'latent_consistency', 'latent_sigreg'):
            if f in used:
                terms[f] = self._normalize_loss(terms[f], update, key=_REG_NORMALIZER_KEYS[f])
                total = total + terms[f] * self.loss_weights[f]
        if not return_intermediates:
            return total
        z = self.zero
        if is_image:
            recon_video = recon_video.squeeze(2)
        t = {f: (v if f in used else z) for f, v in terms.items()}
        return total, VideoTokenizerIntermediates(TokenizerLosses(recon, z, z, z, z, t['latent_ortho'], z, z, t['latent_consistency'], t['latent_sigreg'], z, z),
                                                  recon_video)
