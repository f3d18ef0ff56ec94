"""host-side mirror of the reference's ``vAe()`` Record (reference src/model.py:48-191).

``VAE`` owns the flat device state (parameters, gradients, Adam slots) as PyTorch-ROCm tensors
and drives libargsim_vae.so through the C ABI; PyTorch is plumbing (device memory, streams,
``torch.distributed``), every kernel on the path is hand-written HIP (argsim_amd/csrc).

The reference's feed -> fetch pairs map to methods:
    sess.run(model.train_step)                         -> VAE.train_step(src, tgt)
    sess.run(model.step)                               -> VAE.step
    (errt_samp, loss_gen_samp, loss_kld_samp)          -> VAE.eval(src, tgt)
    model.z.eval({model.src: x})  / encode(sess,vae,x) -> VAE.encode(x) / encode(vae, x)
    decode(sess, vae, z, steps)                        -> VAE.decode(z, steps) / decode(vae, z, steps)
    (new) sampled decoding                             -> VAE.sample(z, ...) / VAE.generate(n, ...) / sample(vae, z, ...)
    (new) importance-weighted log p(x), k draws        -> VAE.score(src, tgt, k, ...) / score(vae, src, k, seed)
    (new) teacher-forced log p(tgt | z)                -> VAE.score_z(z, tgt)
    (new) nearest neighbours among latent rows         -> VAE.neighbors(queries, bank, k, metric) / neighbors(vae, ...)
    (new) aggregate-posterior diagnostics (MI, AU)     -> VAE.posterior_stats(src) / VAE.log_q(z, mu, lv) / VAE.latent_moments(mu, lv)
    (new) linear probes of latent rows (liblinear CV)  -> VAE.probe_fit(z, labels) / VAE.probe_cv(z, labels, folds, groups)
    (new) L1 probes: the useful dimensions (liblinear) -> VAE.probe_fit_l1(z, labels) / VAE.select_dims(z, labels)
    (new) Ward clustering of latent rows (ARS, V_MSR)  -> VAE.ward(z, groups) / VAE.ward_cut(res, k) / VAE.cluster_eval(z, gold, groups)
    (new) affinity propagation of latent rows          -> VAE.affinity(z, metric, ...) / affinity(vae, z, ...)
    (new) k-means of latent rows                       -> VAE.kmeans(z, k, metric, ...) / kmeans(vae, z, k, ...)
    (new) Gaussian mixture of latent rows (BIC, AIC)   -> VAE.gmm(z, k, ...) / VAE.gmm_score(z, model) / VAE.sweep_gmm(z, ks) / generate(prior=)
    (new) exact t-SNE of latent rows                   -> VAE.tsne(z, perplexity, ...) / tsne(vae, z, ...)
    (new) silhouette, CH and DB of many labelings      -> VAE.silhouette(z, labels, metric) / VAE.sweep_k(z, ks) / silhouette(vae, z, ...)
    (new) density clustering of latent rows (DBSCAN)   -> VAE.dbscan(z, eps, min_samples) / VAE.kdist(z, k) / VAE.sweep_eps(z, eps_list)
    (new) principal components of latent rows (PCA)    -> VAE.pca(z, n_components, whiten) / VAE.pca_transform(z, model) / VAE.pca_reduce(z, k)
    (new) kernel two-sample test of latent rows (MMD)  -> VAE.mmd(z, groups) / VAE.mmd2(za, zb) / VAE.prior_match(z) / mmd(vae, z, ...)
"""
import ctypes as C

import numpy as np
import torch

from . import lib as _lib

PARAM, GRAD, ADAM_M, ADAM_V = 0, 1, 2, 3


def _check_cfg(bidirectional, bidir_stacked, attentive, logit_use_embed):
    # reference src/model.py:124-131,136-145,167-168: alternate branches the paper did not train
    # (config.json:17-20); SURVEY section 2.1 marks them out of scope.
    if not (bidirectional and bidir_stacked):
        raise NotImplementedError("only the stacked bidirectional encoder (config.json:17-18) is implemented")
    if attentive:
        raise NotImplementedError("attentive=True is marked 'todo fixme' in the reference (model.py:136) and is not implemented")
    if not logit_use_embed:
        raise NotImplementedError("only tied logits (logit_use_embed=true, config.json:20) are implemented")


class VAE:
    def __init__(self, mode='train', device=0, dim_tgt=8192, dim_emb=512, dim_rep=1024, rnn_layers=3,
                 bidirectional=True, bidir_stacked=True, attentive=False, logit_use_embed=True,
                 accelerate=1e-4, learn_rate=1e-3, bos=2, eos=1, kl_beta=1.0, free_bits=0.0,
                 seed=0, init=True, dtype='f32'):
        assert mode in ('train', 'valid', 'infer')          # model.py:72
        _check_cfg(bidirectional, bidir_stacked, attentive, logit_use_embed)
        if not torch.cuda.is_available():
            raise RuntimeError("argsim_amd needs an MI355X (HIP device): there is no CPU fallback")
        self.mode, self.bos, self.eos = mode, bos, eos
        self.cfg = dict(dim_tgt=dim_tgt, dim_emb=dim_emb, dim_rep=dim_rep, rnn_layers=rnn_layers,
                        accelerate=accelerate, learn_rate=learn_rate, bos=bos, eos=eos)
        self._l = _lib.load()
        self.device = torch.device('cuda', device)
        assert dtype in ('f32', 'bf16', 'f32s'), \
            "dtype: 'f32' (fp32 MFMA, reference), 'f32s' (fp32 via split bf16 MFMA, fp32-accurate) or 'bf16' (bf16 operands in the GEMMs and the GRU recurrence, fp32 accumulate / state)"
        self.dtype = dtype
        c = _lib.AvaeConfig(dim_tgt, dim_emb, dim_rep, rnn_layers, accelerate, learn_rate, bos, eos, 0, 0, kl_beta, free_bits,
                            {'f32': 0, 'bf16': 1, 'f32s': 2}[dtype])
        h = C.c_void_p()
        if self._l.avae_create(C.byref(c), device, C.byref(h)):
            raise RuntimeError("avae_create: " + self._l.avae_last_error(None).decode())
        self._h = h
        n = self._l.avae_state_numel(h)
        with torch.cuda.device(self.device):
            self.state = torch.zeros((4, n), dtype=torch.float32, device=self.device)
        self.params, self.grads, self.adam_m, self.adam_v = (self.state[i] for i in range(4))
        self._ck(self._l.avae_bind_state(h, *(t.data_ptr() for t in (self.params, self.grads, self.adam_m, self.adam_v))))
        self.names = [self._l.avae_param_name(h, i).decode() for i in range(self._l.avae_param_count(h))]
        self.shapes, self.offsets = {}, {}
        for name in self.names:
            off, nd, shp = C.c_int64(), C.c_int32(), (C.c_int64 * 4)()
            self._ck(self._l.avae_param_info(h, name.encode(), C.byref(off), C.byref(nd), shp))
            self.shapes[name] = tuple(shp[i] for i in range(nd.value))
            self.offsets[name] = off.value
        self._hook_ref = None
        self._calls = 0
        self._seed = seed
        if init:
            self.init_params(seed)

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc):
        if rc:
            raise RuntimeError(self._l.avae_last_error(self._h).decode())

    def _stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        self._ck(self._l.avae_set_stream(self._h, C.c_void_p(s)))

    def close(self):
        if getattr(self, '_h', None):
            self._l.avae_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ids(self, x):
        """-> contiguous int32 cuda tensor (B, S)"""
        if isinstance(x, torch.Tensor):       # a pinned host tensor (train.pinned) crosses asynchronously
            return x.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).to(self.device, non_blocking=True)

    def trim(self, x):
        """host twin of util_tf.trim (src/util_tf.py:54-57) on a row-major (B, S') numpy batch:
        drops the all-eos tail columns.  Device tensors are passed through (padding columns are
        masked inside the kernels and cost only time)."""
        if isinstance(x, torch.Tensor):
            if x.is_cuda:
                return x
            m = int((x != self.eos).sum(1).max()) if x.numel() else 0
            return x[:, :max(m, 1)]
        x = np.asarray(x)
        m = int((x != self.eos).sum(1).max()) if x.size else 0
        return x[:, :max(m, 1)]

    # ------------------------------------------------------------------ variables
    def set_tensor(self, name, value, kind=PARAM):
        self._stream()
        t = torch.as_tensor(np.ascontiguousarray(value, dtype=np.float32)).to(self.device)
        assert tuple(t.shape) == self.shapes[name], (name, tuple(t.shape), self.shapes[name])
        self._ck(self._l.avae_set_tensor(self._h, name.encode(), kind, C.c_void_p(t.data_ptr())))
        torch.cuda.current_stream(self.device).synchronize()

    def get_tensor(self, name, kind=PARAM):
        self._stream()
        t = torch.empty(self.shapes[name], dtype=torch.float32, device=self.device)
        self._ck(self._l.avae_get_tensor(self._h, name.encode(), kind, C.c_void_p(t.data_ptr())))
        return t.cpu().numpy()

    def set_params(self, P):
        for k in self.names:
            self.set_tensor(k, P[k])

    def get_params(self, kind=PARAM):
        return {k: self.get_tensor(k, kind) for k in self.names}

    def get_grads(self):
        return self.get_params(GRAD)

    def init_params(self, seed=0):
        """reference initialisers: glorot-uniform kernels (variance_scaling(1.0, fan_avg, uniform),
        model.py:9), zero biases (model.py:8), embedding U(+-sqrt(6/(V/D+1))) (model.py:109-110).
        CudnnGRU draws each gate matrix separately with fan_in = input size, fan_out = num_units."""
        rng = np.random.default_rng(seed)
        V, D = self.cfg['dim_tgt'], self.cfg['dim_emb']
        for name in self.names:
            shp = self.shapes[name]
            if name == 'embed/embedding':
                lim = (6.0 / (V / D + 1.0)) ** 0.5
            elif len(shp) == 1:
                self.set_tensor(name, np.zeros(shp, np.float32))
                continue
            elif name.endswith('/W') or name.endswith('/R'):
                lim = (6.0 / (shp[1] + D)) ** 0.5
            else:
                lim = (6.0 / (shp[0] + shp[1])) ** 0.5
            self.set_tensor(name, rng.uniform(-lim, lim, shp).astype(np.float32))
        self.adam_m.zero_()
        self.adam_v.zero_()

    @property
    def step(self):
        s = C.c_int64()
        self._ck(self._l.avae_get_step(self._h, C.byref(s)))
        return s.value

    @step.setter
    def step(self, v):
        self._ck(self._l.avae_set_step(self._h, int(v)))

    def schedule(self):
        """(rate_keepwd, rate_anneal, rate_update) at the current step (model.py:78-80)"""
        out = (C.c_float * 3)()
        self._ck(self._l.avae_get_schedule(self._h, out))
        return tuple(out)

    def set_option(self, key, value):
        self._ck(self._l.avae_set_option(self._h, key.encode(), int(value)))

    def timing_collect(self):
        """{class: (ms, launches, flops)} from the HIP events recorded while option 'timing' was on"""
        out = (C.c_double * 9)()
        self._stream()
        self._ck(self._l.avae_timing_collect(self._h, out))
        return {k: (out[3 * i], int(out[3 * i + 1]), out[3 * i + 2]) for i, k in enumerate(('gemm', 'gru_fwd', 'gru_bwd'))}

    def present_ids(self):
        """(src, tgt): distinct ids in the last forward's encoder / decoder input where that layer was table-fed, else -1"""
        out = (C.c_int32 * 2)()
        self._stream()
        self._ck(self._l.avae_debug_present_ids(self._h, out))
        return int(out[0]), int(out[1])

    def step_route(self):
        """the route the last forward_backward / train_step took, as the step noted it (test hook avae_debug_step_route) -> dict:
        table (src, tgt) first layers table-fed, compact (encoder, decoder), Bx, bwd_rs (the BPTT form taken: 0 gather, 1
        reduce-scatter), top1 (the top encoder layer as one-job launches + the one-step kernels) and, per kind of GRU launch
        (ROUTE_GRU), the plan it ran as (form, T, C, pipe, ring) or None where the step makes no such launch"""
        out = (C.c_int32 * ROUTE_INTS)()
        self._ck(self._l.avae_debug_step_route(self._h, out))
        return route_dict(list(out))

    def row_expect(self):
        """(source rows, decoder rows, decoder tokens) the last call expected behind its compact layout -- an earlier call's fill scaled to
        its own rows; zeros where it took no layout (test hook avae_debug_row_expect)"""
        out = (C.c_int32 * 3)()
        self._ck(self._l.avae_debug_row_expect(self._h, out))
        return tuple(out)

    def train_ce(self, max_n=1 << 22):
        """per-token cross-entropy (loss_gen_samp, model.py:180) of the last forward_backward / train_step: the TRAIN forward,
        dropout and the latent draw live (test hook)"""
        buf = torch.empty(max_n, dtype=torch.float32, device=self.device)
        n = C.c_int32()
        self._stream()
        self._ck(self._l.avae_debug_train_ce(self._h, C.c_void_p(buf.data_ptr()), max_n, C.byref(n)))
        torch.cuda.synchronize(self.device)
        return buf[:n.value].cpu().numpy()

    def buckets(self):
        out = []
        for i in range(self._l.avae_bucket_count(self._h)):
            o, c = C.c_int64(), C.c_int64()
            self._l.avae_bucket_info(self._h, i, C.byref(o), C.byref(c))
            out.append((o.value, c.value))
        return out

    def set_grad_hook(self, fn):
        """fn(bucket, offset, count) is called while backward is being enqueued (data parallel)."""
        if fn is None:
            self._hook_ref = None
            self._ck(self._l.avae_set_grad_hook(self._h, _lib.GRAD_HOOK(), None))
            return
        self._hook_ref = _lib.GRAD_HOOK(lambda user, b, o, c: fn(b, o, c))
        self._ck(self._l.avae_set_grad_hook(self._h, self._hook_ref, None))

    # ------------------------------------------------------------------ training
    def next_seed(self):
        """the RNG key the next step would use when none is passed: a function of (seed, step, call count)"""
        return (self._seed * 0x9E3779B1 + self.step * 1000003 + self._calls) & 0xFFFFFFFFFFFFFFFF

    def _rng_args(self, seed, keep_mask, eps):
        if seed is None:
            seed = self.next_seed()
        self._calls += 1
        km = ep = None
        if keep_mask is not None:
            km = torch.as_tensor(np.ascontiguousarray(keep_mask)).to(torch.uint8).to(self.device).contiguous()
        if eps is not None:
            ep = torch.as_tensor(np.ascontiguousarray(eps, dtype=np.float32)).to(self.device).contiguous()
        return seed, km, ep

    def forward_backward(self, src, tgt, seed=None, keep_mask=None, eps=None, n_tok_global=0.0, b_global=0.0):
        """gradients of the ELBO into ``self.grads`` (model.py:75-185 + autodiff of minimize())."""
        src, tgt = self._ids(self.trim(src)), self._ids(self.trim(tgt))
        seed, km, ep = self._rng_args(seed, keep_mask, eps)
        if km is not None:
            assert tuple(km.shape) == (tgt.shape[1], tgt.shape[0]), "keep_mask is (S_tgt, B) time-major"
        self._stream()
        self._keep = (src, tgt, km, ep)
        self._ck(self._l.avae_forward_backward(
            self._h, C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()), src.shape[0], src.shape[1], tgt.shape[1],
            C.c_uint64(seed), C.c_void_p(km.data_ptr()) if km is not None else None,
            C.c_void_p(ep.data_ptr()) if ep is not None else None, float(n_tok_global), float(b_global)))

    def adam_step(self):
        """tf.train.AdamOptimizer(rate_update) apply + global_step += 1 (model.py:189)"""
        self._stream()
        self._ck(self._l.avae_adam_step(self._h))

    def train_step(self, src, tgt, seed=None, keep_mask=None, eps=None):
        """sess.run(model_train.train_step)  (src/train.py:118)"""
        self.forward_backward(src, tgt, seed, keep_mask, eps)
        self.adam_step()

    def losses(self):
        """(loss_gen, loss_kld, loss) of the last forward; synchronises"""
        self._stream()
        out = (C.c_float * 3)()
        self._ck(self._l.avae_get_losses(self._h, out))
        return tuple(out)

    # ------------------------------------------------------------------ validation / inference
    def eval(self, src, tgt):
        """(errt_samp (N,), loss_gen_samp (N,), loss_kld_samp (B,R)) in 'valid' mode (src/train.py:109-110)"""
        src, tgt = self._ids(self.trim(src)), self._ids(self.trim(tgt))
        B, R = src.shape[0], self.cfg['dim_rep']
        rt = B * (tgt.shape[1] + 1)
        errt = torch.empty(rt, dtype=torch.float32, device=self.device)
        lgen = torch.empty(rt, dtype=torch.float32, device=self.device)
        lkld = torch.empty((B, R), dtype=torch.float32, device=self.device)
        n = C.c_int32()
        self._stream()
        self._ck(self._l.avae_eval(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(tgt.data_ptr()), B, src.shape[1], tgt.shape[1],
                                   C.c_void_p(errt.data_ptr()), C.c_void_p(lgen.data_ptr()), C.c_void_p(lkld.data_ptr()), C.byref(n)))
        return errt[:n.value].cpu().numpy(), lgen[:n.value].cpu().numpy(), lkld.cpu().numpy()

    def encode(self, src, return_lv=False):
        """latent states z = mu (b, dim_rep) float32 (model.py:194-201)"""
        src = self._ids(self.trim(src))
        b, R = src.shape[0], self.cfg['dim_rep']
        z = torch.empty((b, R), dtype=torch.float32, device=self.device)
        lv = torch.empty((b, R), dtype=torch.float32, device=self.device) if return_lv else None
        self._stream()
        self._ck(self._l.avae_encode(self._h, C.c_void_p(src.data_ptr()), b, src.shape[1], C.c_void_p(z.data_ptr()),
                                     C.c_void_p(lv.data_ptr()) if lv is not None else None))
        z = z.cpu().numpy()
        return (z, lv.cpu().numpy()) if return_lv else z

    def decode_init(self, z):
        """state_in (L, b, D) from z (model.py:156,159,213)"""
        z = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).to(self.device)
        b = z.shape[0]
        s = torch.empty((self.cfg['rnn_layers'], b, self.cfg['dim_emb']), dtype=torch.float32, device=self.device)
        self._stream()
        self._ck(self._l.avae_decode_init(self._h, C.c_void_p(z.data_ptr()), b, C.c_void_p(s.data_ptr())))
        return s

    def decode_step(self, lead, state_in):
        """(pred (1,b) int32, state_ex (L,b,D)) for lead (1,b), one GRU step (model.py:216)"""
        lead = torch.as_tensor(lead).to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        b = lead.shape[0]
        pred = torch.empty(b, dtype=torch.int32, device=self.device)
        out = torch.empty_like(state_in)
        self._stream()
        self._ck(self._l.avae_decode_step(self._h, C.c_void_p(lead.data_ptr()), C.c_void_p(state_in.data_ptr()), b,
                                          C.c_void_p(pred.data_ptr()), C.c_void_p(out.data_ptr())))
        return pred.view(1, b), out

    def decode(self, z, steps=256):
        """greedy decoding, array i32 (b, t<=steps) (model.py:204-219)"""
        z = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).to(self.device)
        b = z.shape[0]
        out = torch.empty((b, steps), dtype=torch.int32, device=self.device)
        n = C.c_int32()
        self._stream()
        self._ck(self._l.avae_decode_greedy(self._h, C.c_void_p(z.data_ptr()), b, steps, C.c_void_p(out.data_ptr()), C.byref(n)))
        return out[:, :n.value].cpu().numpy()


    def sample(self, z, steps=256, temperature=1.0, top_k=0, seed=0, return_logp=False, top_p=0.0, return_nkept=False):
        """sampled decoding (include/argsim_vae.h, avae_decode_sample): array i32 (b, t<=steps) drawn from softmax(logits / temperature)
        over the top_k most likely pieces (0: all), reproducible from seed; a row is eos from its first eos on.  temperature 0 or
        top_k 1 is the argmax.  With return_logp also f32 (b, min(t + 1, steps)): the log-probability of every token, the closing eos
        included (column t for the longest rows), 0 behind it -- a row's sum is the log-probability of its sentence.
        0 < top_p < 1 (avae_decode_sample_p): of those pieces only the nucleus, the most likely ones that hold top_p of the mass; 0 or
        >= 1 is off.  With return_nkept also i32, shaped as logp: the size of the kept set at every position, 0 behind a row's eos,
        -1 everywhere when the nucleus is off."""
        steps, top_k, seed = _check_sample_args(steps, temperature, top_k, seed)
        top_p = _check_top_p(top_p)
        z = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).to(self.device)
        if z.dim() != 2 or z.shape[1] != self.cfg['dim_rep'] or z.shape[0] < 1:
            raise ValueError("z must be (b, dim_rep) with b >= 1, got %s" % (tuple(z.shape),))
        b = z.shape[0]
        out = torch.empty((b, steps), dtype=torch.int32, device=self.device)
        logp = torch.empty((b, steps), dtype=torch.float32, device=self.device) if return_logp else None
        n = C.c_int32()
        self._stream()
        if 0.0 < top_p < 1.0 or return_nkept:
            nkept = torch.empty((b, steps), dtype=torch.int32, device=self.device) if return_nkept else None
            sc = _lib.AvaeSamplePConfig(float(temperature), top_k, seed, top_p, 0)
            self._ck(self._l.avae_decode_sample_p(self._h, C.c_void_p(z.data_ptr()), b, steps, C.byref(sc), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(logp.data_ptr()) if return_logp else None,
                                                  C.c_void_p(nkept.data_ptr()) if return_nkept else None, C.byref(n)))
        else:
            sc = _lib.AvaeSampleConfig(float(temperature), top_k, seed)
            self._ck(self._l.avae_decode_sample(self._h, C.c_void_p(z.data_ptr()), b, steps, C.byref(sc), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(logp.data_ptr()) if return_logp else None, C.byref(n)))
        res = [out[:, :n.value].cpu().numpy()]
        if return_logp:
            res.append(logp[:, :min(n.value + 1, steps)].cpu().numpy())
        if return_nkept:
            res.append(nkept[:, :min(n.value + 1, steps)].cpu().numpy())
        return tuple(res) if len(res) > 1 else res[0]

    def beam(self, z, steps=256, width=4, length_alpha=0.0, return_all=False):
        """beam-search decoding (include/argsim_vae.h, avae_decode_beam): the `width` best continuations per sentence, ranked by
        cum / len ** length_alpha.  By default array i32 (b, t<=steps): the best hypothesis of every row, trimmed as decode() trims.
        With return_all a dict: ids (b, width, n) best first, score, cum (b, width) f32, len (b, width) i32 (tokens including the
        closing eos of a finished hypothesis), n (steps the search ran) and the search lattice lat_parent, lat_token i32, lat_cum f32
        (n, b, width), time-major, in search-slot order."""
        steps, width, length_alpha = _check_beam_args(steps, width, length_alpha)
        if width > self.cfg['dim_tgt']:
            raise ValueError("width must be at most dim_tgt = %d, got %d" % (self.cfg['dim_tgt'], width))
        z = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).to(self.device)
        if z.dim() != 2 or z.shape[1] != self.cfg['dim_rep'] or z.shape[0] < 1:
            raise ValueError("z must be (b, dim_rep) with b >= 1, got %s" % (tuple(z.shape),))
        b = z.shape[0]
        i32, f32 = dict(dtype=torch.int32, device=self.device), dict(dtype=torch.float32, device=self.device)
        out = torch.empty((b, width, steps), **i32)
        score = cum = ln = lp = lt = lc = None
        if return_all:
            score, cum, ln = torch.empty((b, width), **f32), torch.empty((b, width), **f32), torch.empty((b, width), **i32)
            lp, lt, lc = torch.empty((steps, b, width), **i32), torch.empty((steps, b, width), **i32), torch.empty((steps, b, width), **f32)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        n = C.c_int32()
        bc = _lib.AvaeBeamConfig(width, length_alpha)
        self._stream()
        self._ck(self._l.avae_decode_beam(self._h, ptr(z), b, steps, C.byref(bc), ptr(out), ptr(score), ptr(cum), ptr(ln), ptr(lp), ptr(lt),
                                          ptr(lc), C.byref(n)))
        n = n.value
        if not return_all:
            best = out[:, 0, :n].cpu().numpy()
            m = int((best != self.eos).sum(1).max()) if best.size else 0        # (an unfinished best row keeps all n tokens)
            return best[:, :m]
        return dict(ids=out[:, :, :n].cpu().numpy(), score=score.cpu().numpy(), cum=cum.cpu().numpy(), len=ln.cpu().numpy(), n=n,
                    lat_parent=lp[:n].cpu().numpy(), lat_token=lt[:n].cpu().numpy(), lat_cum=lc[:n].cpu().numpy())

    def generate(self, n, steps=256, temperature=1.0, top_k=0, seed=0, return_logp=False, top_p=0.0, prior=None):
        """n sentences from the prior: z ~ N(0, I) drawn on the host with np.random.default_rng(seed), then sample() with the same seed.
        prior: a mixture model of VAE.gmm over the codes -- z is then drawn from it (gmm.sample: the component by choice(p=weights),
        then mean + sqrt(cov) * standard_normal, from the same generator)"""
        if int(n) != n or n < 1:
            raise ValueError("n must be an integer >= 1, got %r" % (n,))
        _check_sample_args(steps, temperature, top_k, seed)
        _check_top_p(top_p)
        z = self.prior_draw(n, seed, prior)
        return self.sample(z, steps, temperature, top_k, seed, return_logp, top_p)

    def prior_draw(self, n, seed=0, prior=None):
        """the z (n, dim_rep) float32 that generate() decodes: N(0, I), or rows of the mixture model `prior`"""
        if prior is None:
            return np.random.default_rng(seed).standard_normal((int(n), self.cfg['dim_rep'])).astype(np.float32)
        from . import gmm
        if np.shape(prior.get('means', ()))[1:] != (self.cfg['dim_rep'],):
            raise ValueError("prior must be a mixture model over dim_rep = %d columns (VAE.gmm)" % self.cfg['dim_rep'])
        return gmm.sample(prior, n, seed)[0]


    # ------------------------------------------------------------------ likelihood
    def score(self, src, tgt=None, k=1, seed=0, eps=None, return_parts=False):
        """k-sample importance-weighted bound on log p(tgt row) with the proposal q(z | src row) (include/argsim_vae.h, avae_score):
        f32 (B,), nats per sentence; tgt=None scores src itself.  The encoder runs once, the k draws go through the decoder as rows.
        eps (k, B, R) overrides the generator (stream 4, reproducible from seed).  With return_parts a dict: bound (B,), logw (k, B),
        logpx (k, B) = log p(tgt | z_k), ntok (B,) positions scored per row (its length + 1), eps (k, B, R) the draws used;
        logw.mean(0) is the k-sample ELBO estimate, exp(-bound.sum() / ntok.sum()) the per-token perplexity."""
        k, seed = _check_score_args(k, seed)
        src = self._ids(self.trim(src))
        tgt = src if tgt is None else self._ids(self.trim(tgt))
        B, R = src.shape[0], self.cfg['dim_rep']
        if src.dim() != 2 or tgt.dim() != 2 or tgt.shape[0] != B or B < 1:
            raise ValueError("src and tgt must be (B, S) with the same B >= 1, got %s and %s" % (tuple(src.shape), tuple(tgt.shape)))
        ep = None
        if eps is not None:
            ep = torch.as_tensor(np.ascontiguousarray(eps, dtype=np.float32)).to(self.device).contiguous()
            if tuple(ep.shape) != (k, B, R):
                raise ValueError("eps must be (k, B, dim_rep) = %s, got %s" % ((k, B, R), tuple(ep.shape)))
        f32 = dict(dtype=torch.float32, device=self.device)
        bound = torch.empty(B, **f32)
        logw = logpx = eps_out = ntok = None
        if return_parts:
            logw, logpx, eps_out = torch.empty((k, B), **f32), torch.empty((k, B), **f32), torch.empty((k, B, R), **f32)
            ntok = torch.empty(B, dtype=torch.int32, device=self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        sc = _lib.AvaeScoreConfig(k, seed)
        self._stream()
        self._ck(self._l.avae_score(self._h, ptr(src), ptr(tgt), B, src.shape[1], tgt.shape[1], C.byref(sc), ptr(ep), ptr(eps_out),
                                    ptr(logpx), ptr(logw), ptr(bound), ptr(ntok)))
        if not return_parts:
            return bound.cpu().numpy()
        return dict(bound=bound.cpu().numpy(), logw=logw.cpu().numpy(), logpx=logpx.cpu().numpy(), ntok=ntok.cpu().numpy(),
                    eps=eps_out.cpu().numpy())

    def score_z(self, z, tgt):
        """teacher-forced log p(tgt row | z row) (avae_score_z), the inverse of sample(): (logpx f32 (b,), ntok i32 (b,)) -- the sum
        of the log-probabilities of the row's tokens and its closing eos, and how many positions that is"""
        z = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float32)).to(self.device)
        tgt = self._ids(self.trim(tgt))
        if z.dim() != 2 or z.shape[1] != self.cfg['dim_rep'] or z.shape[0] < 1 or tgt.dim() != 2 or tgt.shape[0] != z.shape[0]:
            raise ValueError("z must be (b, dim_rep) and tgt (b, S) with b >= 1, got %s and %s" % (tuple(z.shape), tuple(tgt.shape)))
        b = z.shape[0]
        logpx = torch.empty(b, dtype=torch.float32, device=self.device)
        ntok = torch.empty(b, dtype=torch.int32, device=self.device)
        self._stream()
        self._ck(self._l.avae_score_z(self._h, C.c_void_p(z.data_ptr()), C.c_void_p(tgt.data_ptr()), b, tgt.shape[1],
                                      C.c_void_p(logpx.data_ptr()), C.c_void_p(ntok.data_ptr())))
        return logpx.cpu().numpy(), ntok.cpu().numpy()


    # ------------------------------------------------------------------ retrieval
    def neighbors(self, queries, bank, k=10, metric='cos', exclude_self=False, block=None, return_distance=False):
        """the k nearest bank rows of every query row (include/argsim_vae.h, avae_knn) -> (idx int64 (n, k), score float32 (n, k)),
        best first: score descending, ties to the lower index; slots beyond the admissible rows hold -1 / -inf.
        queries (n, dim) and bank (N, dim) are float32 numpy arrays or torch tensors, dim a multiple of 4 up to 1024 (any width, not
        only dim_rep).  A tensor on this device is used in place; a host bank is uploaded in blocks of `block` rows (default: 256 MB
        worth) and searched block by block with the carried list, which gives the same bits as one call; `block` also cuts a
        device bank.  metric: 'dot', 'cos' or 'euc' -- the score of 'euc' is MINUS the squared distance (larger is better, as for
        the others); with return_distance=True the second array is the squared distance itself (+inf in missing slots).
        exclude_self: queries are rows of the bank and a row must not return itself -- True when queries is bank[0:n], an integer
        i0 (or a 1-tuple (i0,)) when it is bank[i0:i0 + n].  The result is numpy, or tensors on the device when queries is a torch
        tensor."""
        k, mid, i0, block = _check_knn_args(queries, bank, k, metric, exclude_self, block)
        if return_distance and mid != 2:
            raise ValueError("return_distance needs metric 'euc', got %r" % (metric,))
        as_torch = isinstance(queries, torch.Tensor)
        dev = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.array(x, order='C'))).to(self.device).contiguous()
        q = dev(queries)
        n, dim, N = q.shape[0], q.shape[1], bank.shape[0]
        on_dev = isinstance(bank, torch.Tensor) and bank.is_cuda
        if block is None:
            block = max(N, 1) if on_dev else max(1, (256 << 20) // (4 * dim))
        idx = torch.empty((n, k), dtype=torch.int64, device=self.device)
        score = torch.empty((n, k), dtype=torch.float32, device=self.device)
        self._stream()
        for j, b0 in enumerate(range(0, max(N, 1), block)):
            part = dev(bank[b0:b0 + block])
            kc = _lib.AvaeKnnConfig(k, mid, b0, i0, 1 if j else 0, 0)
            self._ck(self._l.avae_knn(self._h, C.c_void_p(q.data_ptr()), n, C.c_void_p(part.data_ptr()), part.shape[0], dim, C.byref(kc),
                                      C.c_void_p(idx.data_ptr()), C.c_void_p(score.data_ptr())))
            if not on_dev:
                torch.cuda.current_stream(self.device).synchronize()      # the uploaded block is freed when `part` goes
        if return_distance:
            score = 0.0 - score
        return (idx, score) if as_torch else (idx.cpu().numpy(), score.cpu().numpy())

    # ------------------------------------------------------------------ aggregate-posterior diagnostics
    def _encode_dev(self, src):
        """encode() whose results stay on the device: (mu, lv) float32 tensors (b, dim_rep)"""
        src = self._ids(self.trim(src))
        b, R = src.shape[0], self.cfg['dim_rep']
        mu = torch.empty((b, R), dtype=torch.float32, device=self.device)
        lv = torch.empty((b, R), dtype=torch.float32, device=self.device)
        self._stream()
        self._ck(self._l.avae_encode(self._h, C.c_void_p(src.data_ptr()), b, src.shape[1], C.c_void_p(mu.data_ptr()), C.c_void_p(lv.data_ptr())))
        return mu, lv

    def _dev_f32(self, x):
        return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.array(x, order='C'))).to(self.device).contiguous()

    def latent_moments(self, mu, lv):
        """per-dimension moments of the posteriors N(mu_i, diag exp(lv_i)) over the N rows (include/argsim_vae.h, avae_latent_moments)
        -> dict of float32 (dim,): mean (of mu), var (unbiased variance of mu, 0 for N = 1: a unit is active where it exceeds a
        threshold), sigma2 (mean of exp(lv)) and kl_dim (mean of 1/2 (mu^2 + exp(lv) - lv - 1)).  mu and lv are (N, dim) float32 numpy
        arrays or torch tensors, dim a multiple of 4 up to 1024; the result is numpy, or tensors on the device when mu is a tensor."""
        _check_agg_args(mu, mu, lv, None)
        as_torch = isinstance(mu, torch.Tensor)
        mu, lv = self._dev_f32(mu), self._dev_f32(lv)
        N, dim = mu.shape
        out = torch.empty((4, dim), dtype=torch.float32, device=self.device)
        self._stream()
        self._ck(self._l.avae_latent_moments(self._h, C.c_void_p(mu.data_ptr()), C.c_void_p(lv.data_ptr()), N, dim, C.c_void_p(out.data_ptr())))
        if not as_torch:
            out = out.cpu().numpy()
        return dict(mean=out[0], var=out[1], sigma2=out[2], kl_dim=out[3])

    def log_q(self, z, mu, lv, self_index=None):
        """log-density of every row of z (n, dim) under the aggregate posterior 1/N sum_j N(mu_j, diag exp(lv_j)) of the N rows of
        mu, lv (include/argsim_vae.h, avae_agg_logq) -> logq float32 (n,).  self_index = i0 (True: 0): row i of z was drawn from
        bank row i0 + i, and the result is (logq, logqx) with logqx[i] = log N(z_i; mu_{i0+i}, diag exp(lv_{i0+i})), the own pair's
        term as it entered the sum.  Arrays are float32 numpy or torch, dim a multiple of 4 up to 1024 (any width, not only
        dim_rep); the result is numpy, or tensors on the device when z is a tensor."""
        i0 = _check_agg_args(z, mu, lv, self_index)
        as_torch = isinstance(z, torch.Tensor)
        z, mu, lv = self._dev_f32(z), self._dev_f32(mu), self._dev_f32(lv)
        n, dim, N = z.shape[0], z.shape[1], mu.shape[0]
        logq = torch.empty(n, dtype=torch.float32, device=self.device)
        logqx = torch.empty(n, dtype=torch.float32, device=self.device) if i0 >= 0 else None
        ac = _lib.AvaeAggConfig(i0, (C.c_int32 * 2)(0, 0))
        self._stream()
        self._ck(self._l.avae_agg_logq(self._h, C.c_void_p(z.data_ptr()), n, C.c_void_p(mu.data_ptr()), C.c_void_p(lv.data_ptr()), N, dim,
                                       C.byref(ac), C.c_void_p(logq.data_ptr()), C.c_void_p(logqx.data_ptr()) if logqx is not None else None))
        if not as_torch:
            logq, logqx = logq.cpu().numpy(), (logqx.cpu().numpy() if logqx is not None else None)
        return logq if logqx is None else (logq, logqx)

    def posterior_stats(self, src, samples=1, seed=0, eps=None, batch=128, au_threshold=0.01, return_parts=False):
        """whether the code carries information, over the N sentences of src (ids (N, S)): encodes in batches of `batch` rows (mu
        and lv stay on the device), draws z = mu + exp(lv / 2) eps `samples` times per sentence -- eps is the caller's
        (samples, N, dim_rep) array, or float32 values of numpy.random.default_rng(seed).standard_normal -- and returns a dict:
            kl           sum_j kl_dim: the mean KL(q(z | x) || p(z)) per sentence, in nats
            kl_dim       (R,) its share per latent dimension;  var_mu (R,) the unbiased variance of the posterior mean over the data
            au           active units: how many dimensions have var_mu > au_threshold (Burda et al.)
            mi           mean(logqx - logq): the mutual information I(x; z) under the encoder, at most log N (Hoffman & Johnson)
            kl_marginal  mean(logq - logp): KL(q(z) || p(z)), p the standard normal;  in expectation kl = mi + kl_marginal
            n            N
        with return_parts also the per-sample arrays logq, logqx, logp (samples, N) and z (samples, N, R), and mu, lv (N, R)."""
        samples, seed, batch, thr = _check_stats_args(samples, seed, batch, au_threshold)
        src = np.asarray(src) if not isinstance(src, torch.Tensor) else src
        if len(src.shape) != 2 or src.shape[0] < 1:
            raise ValueError("src must be (N, S) with N >= 1, got %s" % (tuple(src.shape),))
        N, R = src.shape[0], self.cfg['dim_rep']
        if R % 4 or R > 1024:
            raise ValueError("posterior_stats needs dim_rep a multiple of 4 up to 1024, got %d" % R)
        if eps is None:
            eps = np.random.default_rng(seed).standard_normal((samples, N, R), dtype=np.float32)
        ep = torch.as_tensor(np.ascontiguousarray(eps, dtype=np.float32)).to(self.device).contiguous()
        if tuple(ep.shape) != (samples, N, R):
            raise ValueError("eps must be (samples, N, dim_rep) = %s, got %s" % ((samples, N, R), tuple(ep.shape)))
        mu = torch.empty((N, R), dtype=torch.float32, device=self.device)
        lv = torch.empty((N, R), dtype=torch.float32, device=self.device)
        for b0 in range(0, N, batch):
            mu[b0:b0 + batch], lv[b0:b0 + batch] = self._encode_dev(src[b0:b0 + batch])
        mom = self.latent_moments(mu, lv)
        z = mu[None] + torch.exp(0.5 * lv)[None] * ep
        logq = torch.empty((samples, N), dtype=torch.float32, device=self.device)
        logqx = torch.empty((samples, N), dtype=torch.float32, device=self.device)
        for s in range(samples):
            logq[s], logqx[s] = self.log_q(z[s], mu, lv, self_index=0)
        logp = -0.5 * (z.double() ** 2).sum(-1) - 0.5 * R * float(np.log(2.0 * np.pi))
        kl_dim, var_mu = mom['kl_dim'].cpu().numpy(), mom['var'].cpu().numpy()
        res = dict(kl=float(kl_dim.astype(np.float64).sum()), kl_dim=kl_dim, var_mu=var_mu, au=int((var_mu > thr).sum()),
                   mi=float((logqx.double() - logq.double()).mean()), kl_marginal=float((logq.double() - logp).mean()), n=N)
        if return_parts:
            res.update(logq=logq.cpu().numpy(), logqx=logqx.cpu().numpy(), logp=logp.cpu().numpy(), z=z.cpu().numpy(),
                       mu=mu.cpu().numpy(), lv=lv.cpu().numpy())
        return res

    def probe_fit(self, z, labels, C=0.001, class_weight='balanced', train=None, **solver):
        """a one-vs-rest L2 logistic regression on the rows `train` (all rows: None) of z (N, dim), the model of scikit-learn's
        LogisticRegression(C, solver='liblinear', class_weight) fitted on the device (include/argsim_vae.h, avae_probe_fit) -> an
        object with classes_, coef_, intercept_, stats, decision(z) and predict(z) (argsim_amd/probe.py).  solver: tol, max_newton,
        max_cg."""
        from . import probe
        return probe.fit(self, z, labels, C, class_weight, train, **solver)

    def probe_cv(self, z, labels, folds, groups=None, C=0.001, class_weight='balanced', **solver):
        """cross-validation of that model: every group x fold x class is one problem of ONE avae_probe_fit over the shared z -> dict
        with pred (N,) the held-out predictions, scores {group: mean micro-F1 over its folds} and mean, the figures the reference's
        src/eval_classification.py prints, and stats (P, 4) of the problems (argsim_amd/probe.py, cross_validate)."""
        from . import probe
        return probe.cross_validate(self, z, labels, folds, groups, C, class_weight, **solver)

    def probe_fit_l1(self, z, labels, C=0.1, class_weight=None, train=None, **solver):
        """the one-vs-rest L1 logistic regression of the reference's src/eval_clustering.py:46, LogisticRegression(penalty='l1', C,
        solver='liblinear'), fitted on the device (include/argsim_vae.h, avae_probe_fit_l1) -> the object probe_fit returns; a zero
        coefficient is an exact 0.  solver: tol, max_newton, max_inner."""
        from . import probe
        return probe.fit_l1(self, z, labels, C, class_weight, train, **solver)

    def select_dims(self, z, labels, C=0.1, class_weight=None, train=None, **solver):
        """the useful dimensions of src/eval_clustering.py:57 -> (dims, probe): the sorted columns of z with a nonzero coefficient in
        any class of that L1 model (int64, as useful_dimension.npy), and the model"""
        from . import probe
        return probe.select_dims(self, z, labels, C, class_weight, train, **solver)

    def ward(self, z, groups=None):
        """the Ward tree (sklearn's AgglomerativeClustering default, scipy's linkage(x, 'ward')) of every group of rows of z, all groups
        in ONE device call (include/argsim_vae.h, avae_ward).  groups: None, an (N,) array of group labels or {key: row numbers}
        -> dict(keys, group_off, groups {key: dict(rows, pair, delta, size, Z)}) (argsim_amd/cluster.py)"""
        from . import cluster
        return cluster.ward(self, z, groups)

    def ward_cut(self, res, k):
        """the clusters of ward's result cut at k clusters per group (avae_ward_cut) -> {key: labels 0 .. k - 1 aligned with the
        group's rows}"""
        from . import cluster
        return cluster.ward_cut(self, res, k)

    def cluster_eval(self, z, gold, groups=None):
        """the reference's clustering evaluation (src/eval_clustering.py:95-102) for every group at once -> {key: (ARS, V_MSR)}: as
        many Ward clusters as the group has distinct gold labels, scored by the adjusted Rand score and the V-measure"""
        from . import cluster
        return cluster.cluster_eval(self, z, gold, groups)

    def affinity(self, z, metric='euclidean', preference=None, damping=0.5, max_iter=200, convergence_iter=15, seed=0, noise=True,
                 return_messages=False):
        """affinity propagation of the rows of z (sklearn's AffinityPropagation; src/eval_clustering_explorative.py:83-103) in ONE
        device call (include/argsim_vae.h, avae_affinity).  metric: 'euclidean' (minus the squared distance), 'cosine' (minus the
        cosine distance) or 'precomputed' (z is the (N, N) similarity matrix); preference None: the median similarity
        -> dict(labels 0 .. K - 1 in ascending exemplar row or all -1, exemplars, n_iter, converged) (argsim_amd/affinity.py)"""
        from . import affinity
        return affinity.affinity(self, z, metric, preference, damping, max_iter, convergence_iter, seed, noise, return_messages)

    def tsne(self, z, perplexity=30.0, max_iter=1000, init='pca', seed=0, learning_rate='auto', early_exaggeration=12.0,
             exaggeration_iter=250, n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, p=None, return_p=False,
             return_trace=False):
        """exact t-SNE of the rows of z into two dimensions (sklearn's TSNE(method='exact'); src/eval_clustering_explorative.py:45-66)
        in ONE device call (include/argsim_vae.h, avae_tsne).  init: 'pca', 'random' (the generator's stream 6 from seed; what the
        reference's sklearn did) or an (N, 2) array; p: the joint matrix of an earlier call with return_p
        -> dict(y, kl, n_iter, stop, and with the flags p, beta, trace) (argsim_amd/tsne.py)"""
        from . import tsne
        return tsne.tsne(self, z, perplexity, max_iter, init, seed, learning_rate, early_exaggeration, exaggeration_iter, n_iter_check,
                         n_iter_without_progress, min_grad_norm, p, return_p, return_trace)

    def kmeans(self, z, k, metric='euclidean', n_init=10, max_iter=300, tol=1e-4, seed=0, init='k-means++', return_all=False):
        """k-means of the rows of z (sklearn's KMeans(algorithm='lloyd'): greedy k-means++ seeding, Lloyd iterations, the relocation of
        empty clusters) with n_init restarts side by side in ONE device call (include/argsim_vae.h, avae_kmeans).  metric: 'euclidean' or
        'cosine' (spherical k-means); init: 'k-means++' or the centres, (k, dim) or (n_init, k, dim)
        -> dict(labels, centers, inertia, n_iter, stop, best, inertias, relocations) (argsim_amd/kmeans.py)"""
        from . import kmeans
        return kmeans.kmeans(self, z, k, metric, n_init, max_iter, tol, seed, init, return_all)

    def silhouette(self, z, labels, metric='euclidean', return_samples=False):
        """sklearn's silhouette_score, calinski_harabasz_score and davies_bouldin_score of the rows of z for every labeling in labels,
        (N,) or (L, N) integers with negative = left out, in ONE device call that forms every pair distance once (include/argsim_vae.h,
        avae_silhouette).  metric: 'euclidean', 'cosine' or 'sqeuclidean'
        -> dict(score, ch, db, n_clusters, counts, clusters[, samples, a, b, nearest]) (argsim_amd/silhouette.py)"""
        from . import silhouette
        return silhouette.silhouette(self, z, labels, metric, return_samples)

    def sweep_k(self, z, ks, metric='euclidean', n_init=10, seed=0):
        """one kmeans call per k in ks, then ONE silhouette call over all the labelings -> dict(k, score, ch, db, inertia, labels, best)"""
        from . import silhouette
        return silhouette.sweep_k(self, z, ks, metric, n_init, seed)

    def gmm(self, z, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0, init='kmeans', return_resp=False,
            return_all=False):
        """Gaussian mixture of the rows of z (sklearn's GaussianMixture with 'diag' or 'spherical' covariances: EM from k-means labels,
        given labels or given parameters) with n_init restarts side by side in ONE device call (include/argsim_vae.h, avae_gmm_fit)
        -> dict(weights, means, covariances, labels, logp, lower_bound, lower_bounds, n_iter, stop, converged, best, n_parameters, bic,
        aic[, resp, *_all, trace]) (argsim_amd/gmm.py)"""
        from . import gmm
        return gmm.gmm(self, z, k, covariance, n_init, max_iter, tol, reg_covar, seed, init, return_resp, return_all)

    def gmm_score(self, z, model, return_resp=False):
        """log p(z_i) of the rows of z under a mixture model of VAE.gmm -> dict(logp, labels[, resp]) (avae_gmm_score)"""
        from . import gmm
        return gmm.gmm_score(self, z, model, return_resp)

    def sweep_gmm(self, z, ks, **kw):
        """one gmm call per k in ks -> dict(k, bic, aic, lower_bound, models, best): best is the k with the smallest BIC"""
        from . import gmm
        return gmm.sweep_gmm(self, z, ks, **kw)

    def dbscan(self, z, eps, min_samples=5, metric='euclidean', max_rounds=0):
        """sklearn's DBSCAN(algorithm='brute') of the rows of z in ONE device call (include/argsim_vae.h, avae_dbscan): no cluster count,
        noise rows at -1, labels an exact function of the rows.  metric: 'euclidean' or 'cosine'
        -> dict(labels, core_sample_indices, n_clusters, n_noise, n_border, counts, rounds) (argsim_amd/dbscan.py)"""
        from . import dbscan
        return dbscan.dbscan(self, z, eps, min_samples, metric, max_rounds)

    def kdist(self, z, k, metric='euclidean'):
        """the ascending curve of every row's distance to its k-th nearest other row: eps is read off its knee"""
        from . import dbscan
        return dbscan.kdist(self, z, k, metric)

    def sweep_eps(self, z, eps_list, min_samples=5, metric='euclidean'):
        """one dbscan call per eps, then ONE silhouette call over the labelings that can be scored (noise left out)
        -> dict(eps, n_clusters, n_noise, score, ch, db, labels, best)"""
        from . import dbscan
        return dbscan.sweep_eps(self, z, eps_list, min_samples, metric)

    def pca(self, z, n_components=None, whiten=False, max_sweeps=0):
        """principal components of the rows of z in ONE device call (include/argsim_vae.h, avae_pca_fit): mean, covariance and Jacobi
        eigen-solve in double, scikit-learn's signs and variances
        -> dict(mean, components, explained_variance, explained_variance_ratio, singular_values, noise_variance, effective_dim,
        n_samples, rank, sweeps, whiten) (argsim_amd/pca.py)"""
        from . import pca
        return pca.pca(self, z, n_components, whiten, max_sweeps)

    def pca_transform(self, z, model):
        """the rows of z in the model's components (whitened if the model says so) -> (n, k) float32"""
        from . import pca
        return pca.transform(self, z, model)

    def pca_reduce(self, z, k, whiten=False):
        """fit + transform: the leading k principal directions of the rows of z -> (y (N, k) float32, model)"""
        from . import pca
        return pca.reduce(self, z, k, whiten)

    def mmd(self, z, groups, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False):
        """do the rows with groups == 0 and those with groups == 1 come from the same distribution?  The unbiased kernel two-sample
        statistic MMD^2_u with a permutation null in ONE device call for every row of groups, (N,) or (G, N) integers (negative: left
        out) (include/argsim_vae.h, avae_mmd).  kernel: 'rbf' or 'energy'; gamma: 'median', a number or up to 8 numbers
        -> dict(stat, pvalue, m, n[, null, witness]) (argsim_amd/mmd.py)"""
        from . import mmd
        return mmd.mmd(self, z, groups, kernel, gamma, metric, n_perm, seed, return_null, return_witness)

    def mmd2(self, za, zb, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False):
        """VAE.mmd for two arrays of rows: za against zb"""
        from . import mmd
        return mmd.mmd2(self, za, zb, kernel, gamma, metric, n_perm, seed, return_null, return_witness)

    def prior_match(self, z, n_perm=999, seed=0):
        """does the aggregate posterior match the prior that generate samples from?  The rows of z against as many N(0, I) rows
        (the InfoVAE diagnostic MMD(q(z), p(z))) -> dict(stat, pvalue, m, n)"""
        from . import mmd
        return mmd.prior_match(self, z, n_perm, seed)


# avae_debug_step_route: seven scalars, then (form, T, C, pipe, ring) per kind of GRU launch, in this order
ROUTE_GRU = ('enc_fwd', 'enc_bwd', 'top_fwd', 'top_bwd', 'dec_fwd', 'dec_bwd')
ROUTE_INTS = 7 + 5 * len(ROUTE_GRU)


def route_dict(v):
    """the ints of avae_debug_step_route as VAE.step_route() returns them (no device needed)"""
    if len(v) != ROUTE_INTS:
        raise ValueError("a step route is %d ints, got %d" % (ROUTE_INTS, len(v)))
    v = [int(x) for x in v]
    r = dict(table=(v[0], v[1]), compact=(v[2], v[3]), Bx=v[4], bwd_rs=v[5], top1=v[6])
    for i, k in enumerate(ROUTE_GRU):
        g = tuple(v[7 + 5 * i:12 + 5 * i])
        r[k] = None if g[0] < 0 else g
    return r


KNN_METRICS = {'dot': 0, 'cos': 1, 'euc': 2}


def _check_knn_args(queries, bank, k, metric, exclude_self=False, block=None):
    """the argument rules of avae_knn, checked before anything touches the device -> (k, metric id, self_base or -1, block or None)"""
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= 32:
        raise ValueError("k must be an integer in [1, 32], got %r" % (k,))
    if not isinstance(metric, str) or metric not in KNN_METRICS:
        raise ValueError("metric must be one of 'dot', 'cos', 'euc', got %r" % (metric,))
    for name, x in (('queries', queries), ('bank', bank)):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise ValueError("%s must be a numpy array or a torch tensor, got %s" % (name, type(x).__name__))
        if x.dtype not in (np.float32, torch.float32):
            raise ValueError("%s must be float32, got %s" % (name, x.dtype))
        if len(x.shape) != 2:
            raise ValueError("%s must be (rows, dim), got %s" % (name, tuple(x.shape)))
    if queries.shape[0] < 1:
        raise ValueError("queries must have at least one row, got %s" % (tuple(queries.shape),))
    dim = queries.shape[1]
    if bank.shape[1] != dim:
        raise ValueError("queries and bank must have the same dim, got %d and %d" % (dim, bank.shape[1]))
    if dim % 4 or not 4 <= dim <= 1024:
        raise ValueError("dim must be a multiple of 4 in [4, 1024], got %d" % (dim,))
    if isinstance(exclude_self, (tuple, list)):
        if len(exclude_self) != 1:
            raise ValueError("exclude_self must be a bool, an integer i0 or (i0,), got %r" % (exclude_self,))
        exclude_self = exclude_self[0]
    if isinstance(exclude_self, (bool, np.bool_)):
        i0 = 0 if exclude_self else -1
    else:
        if int(exclude_self) != exclude_self or exclude_self < 0:
            raise ValueError("exclude_self must be a bool, an integer i0 >= 0 or (i0,), got %r" % (exclude_self,))
        i0 = int(exclude_self)
    if block is not None and (isinstance(block, bool) or int(block) != block or not 1 <= block < (1 << 31) - 256):
        raise ValueError("block must be an integer in [1, 2^31 - 256), got %r" % (block,))
    return int(k), KNN_METRICS[metric], i0, None if block is None else int(block)


def _check_agg_args(z, mu, lv, self_index=None):
    """the argument rules of avae_agg_logq (and, with z = mu, of avae_latent_moments), checked before anything touches the device
    -> self_base (-1: off)"""
    for name, x in (('z', z), ('mu', mu), ('lv', lv)):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise ValueError("%s must be a numpy array or a torch tensor, got %s" % (name, type(x).__name__))
        if x.dtype not in (np.float32, torch.float32):
            raise ValueError("%s must be float32, got %s" % (name, x.dtype))
        if len(x.shape) != 2:
            raise ValueError("%s must be (rows, dim), got %s" % (name, tuple(x.shape)))
        if isinstance(x, torch.Tensor) and x.is_contiguous() and x.data_ptr() % 16:
            raise ValueError("%s must be 16-byte aligned (a view that starts inside a row block is not)" % name)
    if tuple(mu.shape) != tuple(lv.shape):
        raise ValueError("mu and lv must have the same shape, got %s and %s" % (tuple(mu.shape), tuple(lv.shape)))
    n, dim, N = z.shape[0], z.shape[1], mu.shape[0]
    if n < 1 or N < 1:
        raise ValueError("z and mu must have at least one row, got %s and %s" % (tuple(z.shape), tuple(mu.shape)))
    if N > (1 << 31) - 256 or n > (1 << 31) - 256:
        raise ValueError("at most 2^31 - 256 rows per call, got %d and %d" % (n, N))
    if mu.shape[1] != dim:
        raise ValueError("z and mu must have the same dim, got %d and %d" % (dim, mu.shape[1]))
    if dim % 4 or not 4 <= dim <= 1024:
        raise ValueError("dim must be a multiple of 4 in [4, 1024], got %d" % (dim,))
    if self_index is None or self_index is False:
        return -1
    if self_index is True:
        self_index = 0
    if isinstance(self_index, (bool, np.bool_)) or int(self_index) != self_index or self_index < 0:
        raise ValueError("self_index must be None, True or an integer i0 >= 0, got %r" % (self_index,))
    if int(self_index) + n > N:
        raise ValueError("self_index + n = %d exceeds N = %d (row i of z is a sample of bank row self_index + i)" % (int(self_index) + n, N))
    return int(self_index)


def _check_stats_args(samples, seed, batch, au_threshold):
    """the argument rules of VAE.posterior_stats -> (samples, seed, batch, au_threshold)"""
    if isinstance(samples, bool) or int(samples) != samples or not 1 <= samples <= 1 << 20:
        raise ValueError("samples must be an integer in [1, 2^20], got %r" % (samples,))
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    if isinstance(batch, bool) or int(batch) != batch or batch < 1:
        raise ValueError("batch must be an integer >= 1, got %r" % (batch,))
    t = float(au_threshold)
    if not t >= 0.0:
        raise ValueError("au_threshold must be a number >= 0, got %r" % (au_threshold,))
    return int(samples), int(seed), int(batch), t


def _check_score_args(k, seed):
    """the argument rules of avae_score, checked before anything touches the device -> (k, seed) as ints"""
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= 1 << 20:
        raise ValueError("k must be an integer in [1, 2^20], got %r" % (k,))
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    return int(k), int(seed)


def _check_sample_args(steps, temperature, top_k, seed):
    """the argument rules of avae_decode_sample, checked before anything touches the device -> (steps, top_k, seed) as ints"""
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= steps <= 1 << 20:
        raise ValueError("steps must be an integer in [1, 2^20], got %r" % (steps,))
    t = float(temperature)
    if not (t >= 0.0) or t == float('inf'):
        raise ValueError("temperature must be a finite number >= 0, got %r" % (temperature,))
    if isinstance(top_k, bool) or int(top_k) != top_k or not 0 <= top_k < 1 << 31:
        raise ValueError("top_k must be an integer >= 0, got %r" % (top_k,))
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    return int(steps), int(top_k), int(seed)


def _check_top_p(top_p):
    """the rule of avae_decode_sample_p for top_p, checked before anything touches the device -> float (0 or >= 1: the nucleus is off)"""
    if isinstance(top_p, bool):
        raise ValueError("top_p must be a number >= 0, got %r" % (top_p,))
    p = float(top_p)
    if not p >= 0.0:
        raise ValueError("top_p must be a number >= 0, got %r" % (top_p,))
    return p


def _check_beam_args(steps, width, length_alpha):
    """the argument rules of avae_decode_beam, checked before anything touches the device -> (steps, width, length_alpha)"""
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= steps <= 1 << 20:
        raise ValueError("steps must be an integer in [1, 2^20], got %r" % (steps,))
    if isinstance(width, bool) or int(width) != width or not 1 <= width <= 32:
        raise ValueError("width must be an integer in [1, 32], got %r" % (width,))
    a = float(length_alpha)
    if not (a >= 0.0) or a == float('inf'):
        raise ValueError("length_alpha must be a finite number >= 0, got %r" % (length_alpha,))
    return int(steps), int(width), a


def vAe(mode, src=None, tgt=None, **cfg):
    """reference-shaped constructor (src/model.py:48): returns the VAE object in place of the Record.
    ``src``/``tgt`` pipeline tensors have no counterpart: batches are passed to the methods."""
    return VAE(mode, **cfg)


def encode(vae, src):
    """src/model.py:194-201 without the session argument"""
    return vae.encode(src)


def decode(vae, z, steps=256):
    """src/model.py:204-219 without the session argument"""
    return vae.decode(z, steps)


def sample(vae, z, steps=256, temperature=1.0, top_k=0, seed=0, return_logp=False, top_p=0.0):
    """sampled counterpart of decode(): VAE.sample"""
    return vae.sample(z, steps, temperature, top_k, seed, return_logp, top_p)


def beam(vae, z, steps=256, width=4, length_alpha=0.0, return_all=False):
    """beam-search counterpart of decode(): VAE.beam"""
    return vae.beam(z, steps, width, length_alpha, return_all)


def score(vae, src, k=1, seed=0):
    """importance-weighted log p(src row) per sentence, k draws: VAE.score"""
    return vae.score(src, None, k, seed)


def neighbors(vae, queries, bank, k=10, metric='cos', exclude_self=False, block=None, return_distance=False):
    """the k nearest bank rows of every query row: VAE.neighbors"""
    return vae.neighbors(queries, bank, k, metric, exclude_self, block, return_distance)


def latent_moments(vae, mu, lv):
    """per-dimension moments of the posteriors over the rows: VAE.latent_moments"""
    return vae.latent_moments(mu, lv)


def log_q(vae, z, mu, lv, self_index=None):
    """log-density of the rows of z under the aggregate posterior: VAE.log_q"""
    return vae.log_q(z, mu, lv, self_index)


def posterior_stats(vae, src, samples=1, seed=0, eps=None, batch=128, au_threshold=0.01, return_parts=False):
    """active units, mutual information and marginal KL over the sentences of src: VAE.posterior_stats"""
    return vae.posterior_stats(src, samples, seed, eps, batch, au_threshold, return_parts)


def probe_fit(vae, z, labels, C=0.001, class_weight='balanced', train=None, **solver):
    """functional form of VAE.probe_fit"""
    return vae.probe_fit(z, labels, C, class_weight, train, **solver)


def probe_cv(vae, z, labels, folds, groups=None, C=0.001, class_weight='balanced', **solver):
    """functional form of VAE.probe_cv"""
    return vae.probe_cv(z, labels, folds, groups, C, class_weight, **solver)


def probe_fit_l1(vae, z, labels, C=0.1, class_weight=None, train=None, **solver):
    """functional form of VAE.probe_fit_l1"""
    return vae.probe_fit_l1(z, labels, C, class_weight, train, **solver)


def select_dims(vae, z, labels, C=0.1, class_weight=None, train=None, **solver):
    """functional form of VAE.select_dims"""
    return vae.select_dims(z, labels, C, class_weight, train, **solver)


def ward(vae, z, groups=None):
    """functional form of VAE.ward"""
    return vae.ward(z, groups)


def ward_cut(vae, res, k):
    """functional form of VAE.ward_cut"""
    return vae.ward_cut(res, k)


def affinity(vae, z, metric='euclidean', preference=None, damping=0.5, max_iter=200, convergence_iter=15, seed=0, noise=True,
             return_messages=False):
    """functional form of VAE.affinity"""
    return vae.affinity(z, metric, preference, damping, max_iter, convergence_iter, seed, noise, return_messages)


def cluster_eval(vae, z, gold, groups=None):
    """functional form of VAE.cluster_eval"""
    return vae.cluster_eval(z, gold, groups)


def tsne(vae, z, perplexity=30.0, max_iter=1000, init='pca', seed=0, learning_rate='auto', early_exaggeration=12.0, exaggeration_iter=250,
         n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, p=None, return_p=False, return_trace=False):
    """functional form of VAE.tsne"""
    return vae.tsne(z, perplexity, max_iter, init, seed, learning_rate, early_exaggeration, exaggeration_iter, n_iter_check,
                    n_iter_without_progress, min_grad_norm, p, return_p, return_trace)


def _check_kmeans_args(z, k, metric='euclidean', n_init=10, max_iter=300, tol=1e-4, seed=0, init='k-means++'):
    """the argument rules of VAE.kmeans, checked before anything touches the device (ValueError)"""
    from . import kmeans as _km
    return _km._check_kmeans_args(z, k, metric, n_init, max_iter, tol, seed, init)


def kmeans(vae, z, k, metric='euclidean', n_init=10, max_iter=300, tol=1e-4, seed=0, init='k-means++', return_all=False):
    """functional form of VAE.kmeans"""
    return vae.kmeans(z, k, metric, n_init, max_iter, tol, seed, init, return_all)


def silhouette(vae, z, labels, metric='euclidean', return_samples=False):
    """functional form of VAE.silhouette"""
    return vae.silhouette(z, labels, metric, return_samples)


def _check_gmm_args(z, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0, init='kmeans'):
    """the argument rules of VAE.gmm, checked before anything touches the device (ValueError)"""
    from . import gmm as _gm
    return _gm._check_gmm_args(z, k, covariance, n_init, max_iter, tol, reg_covar, seed, init)


def gmm(vae, z, k, covariance='diag', n_init=1, max_iter=100, tol=1e-3, reg_covar=1e-6, seed=0, init='kmeans', return_resp=False,
        return_all=False):
    """functional form of VAE.gmm"""
    return vae.gmm(z, k, covariance, n_init, max_iter, tol, reg_covar, seed, init, return_resp, return_all)


def gmm_score(vae, z, model, return_resp=False):
    """functional form of VAE.gmm_score"""
    return vae.gmm_score(z, model, return_resp)


def sweep_gmm(vae, z, ks, **kw):
    """functional form of VAE.sweep_gmm"""
    return vae.sweep_gmm(z, ks, **kw)


def dbscan(vae, z, eps, min_samples=5, metric='euclidean', max_rounds=0):
    """functional form of VAE.dbscan"""
    return vae.dbscan(z, eps, min_samples, metric, max_rounds)


def kdist(vae, z, k, metric='euclidean'):
    """functional form of VAE.kdist"""
    return vae.kdist(z, k, metric)


def sweep_eps(vae, z, eps_list, min_samples=5, metric='euclidean'):
    """functional form of VAE.sweep_eps"""
    return vae.sweep_eps(z, eps_list, min_samples, metric)


def pca(vae, z, n_components=None, whiten=False, max_sweeps=0):
    """functional form of VAE.pca"""
    return vae.pca(z, n_components, whiten, max_sweeps)


def pca_transform(vae, z, model):
    """functional form of VAE.pca_transform"""
    return vae.pca_transform(z, model)


def pca_reduce(vae, z, k, whiten=False):
    """functional form of VAE.pca_reduce"""
    return vae.pca_reduce(z, k, whiten)


def mmd(vae, z, groups, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False):
    """functional form of VAE.mmd"""
    return vae.mmd(z, groups, kernel, gamma, metric, n_perm, seed, return_null, return_witness)


def mmd2(vae, za, zb, kernel='rbf', gamma='median', metric='euclidean', n_perm=999, seed=0, return_null=False, return_witness=False):
    """functional form of VAE.mmd2"""
    return vae.mmd2(za, zb, kernel, gamma, metric, n_perm, seed, return_null, return_witness)


def prior_match(vae, z, n_perm=999, seed=0):
    """functional form of VAE.prior_match"""
    return vae.prior_match(z, n_perm, seed)
