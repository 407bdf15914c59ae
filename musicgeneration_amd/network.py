"""Host-side mirror of the reference's ``network.py`` (mg/model/MusicTransformer/network.py:14-84).

``MusicTransformer`` keeps the reference's constructor, attributes, ``state_dict`` keys and the
three-way ``forward`` convention (train -> logits; eval -> (logits, weights); after ``test()`` ->
``generate(...).tolist()``), and runs on the HIP kernels of libmgx.so.  There is no eager/CPU
fallback: ``forward`` on a CPU tensor raises.
"""
from __future__ import annotations

import os

from typing import Optional

import torch

from . import config, decode, ops
from .layers import Encoder, EncoderLayer, FlatStore, seed_stride


class MusicTransformer(torch.nn.Module):
    def __init__(self, embedding_dim=256, vocab_size=388 + 2, num_layer=6,
                 max_seq=2048, dropout=0.2, debug=False, loader_path=None, dist=False, writer=None):
        super().__init__()
        self.infer = False
        if loader_path is not None:
            raise NotImplementedError("loader_path: the reference calls an undefined load_config_file "
                                      "(network.py:19-20); pass the hyper-parameters explicitly")
        self._debug = debug
        self.max_seq = max_seq
        self.num_layer = num_layer
        self.embedding_dim = embedding_dim
        self.vocab_size = vocab_size
        self.dist = dist
        self.writer = writer
        self.dropout_rate = dropout
        # the reference reads the pad id from the global config module (network.py:37); the default
        # is the same rule (pad = last vocabulary id), overridable per model
        self.pad_token = vocab_size - 1
        self.vocab_padded = (vocab_size + 63) // 64 * 64     # rows of the vocabulary GEMM (zero rows beyond V)
        if embedding_dim % 64 != 0:
            raise ValueError("the MI355X kernels fix the head width at 64 (the reference's h = d // 64, dh = d // h, layers.py:219): "
                             f"embedding_dim must be a multiple of 64, got {embedding_dim}")
        self.ffn_padded = (embedding_dim // 2 + 63) // 64 * 64      # FFN width in the flat buffers (zero rows / columns beyond d/2)
        self.Decoder = Encoder(num_layers=self.num_layer, d_model=self.embedding_dim,
                               input_vocab_size=self.vocab_size, rate=dropout, max_len=max_seq)
        self.fc = torch.nn.Linear(self.embedding_dim, self.vocab_size)
        self.return_attention_weights = False   # eval-mode [B,h,L,L] weights are a debug output
        self._store: Optional[FlatStore] = None
        self._seed_ctr = 0
        self._dp = None                          # set by dp.DataParallel
        self._pad_flag: Optional[torch.Tensor] = None   # device int32[1], sticky: a row started with padding and held real tokens

    # ------------------------------------------------------------------------------------------
    # flat storage
    # ------------------------------------------------------------------------------------------
    def _flat_order(self):
        named = dict(self.named_parameters())
        order = ["Decoder.embedding.weight"]
        buckets = [("embedding", ["Decoder.embedding.weight"])]
        for i in range(self.num_layer):
            names = [f"Decoder.enc_layers.{i}.{n}" for n in EncoderLayer.FLAT_ORDER]
            order += names
            buckets.append((f"layer{i}", names))
        order += ["fc.weight", "fc.bias"]
        buckets.append(("fc", ["fc.weight", "fc.bias"]))
        assert set(order) == set(named), "flat order must cover every parameter exactly once"
        padded = {"fc.weight": self.vocab_padded * self.embedding_dim, "fc.bias": self.vocab_padded}
        # FFN width d/2 (layers.py:143-144) padded to the GEMMs' reduction granule of 64 when d = 64 * odd (d = 192, 320, ...): zero
        # rows / bias entries of FFN_pre, zero columns of FFN_suf -- ReLU(0) = 0 feeds zero columns, every gradient there is exactly 0,
        # Adam leaves zeros zero.  The Parameters keep the reference's shapes (state_dict, checkpoints).
        colpad = {}
        H, Hp, d = self.embedding_dim // 2, self.ffn_padded, self.embedding_dim
        if Hp != H:
            for i in range(self.num_layer):
                pre = f"Decoder.enc_layers.{i}."
                padded[pre + "FFN_pre.weight"] = Hp * d
                padded[pre + "FFN_pre.bias"] = Hp
                colpad[pre + "FFN_suf.weight"] = Hp
        return [(n, named[n]) for n in order], buckets, padded, colpad

    def store(self) -> FlatStore:
        dev = self.fc.weight.device
        if self._store is None or self._store.param.device != dev:
            if dev.type != "cuda":
                raise ops._lib.MgxError("MusicTransformer runs on the MI355X kernels only: move it to a HIP "
                                        "device first (model.to('cuda')); there is no CPU fallback")
            named, buckets, padded, colpad = self._flat_order()
            self._store = FlatStore(named, dev, buckets, padded, colpad)
            if os.environ.get("MGX_DETERMINISTIC", "0") == "1" and not ops.deterministic():
                ops.set_deterministic(True, dev)
        return self._store

    def _apply(self, fn, *a, **k):     # .to()/.cuda() re-materialise parameters: rebuild lazily
        self._store = None
        return super()._apply(fn, *a, **k)

    def _next_seed(self) -> int:
        # under data parallelism every rank usually calls torch.manual_seed with the same value: the rank enters the seed, or
        # all ranks would draw the same dropout masks for their (different) rows.  One call uses seed .. seed + 4 * num_layer - 2
        # (_hidden), so consecutive calls lie seed_stride apart: 64 up to 16 layers, more beyond
        self._seed_ctr += 1
        rank = self._dp.rank if self._dp is not None else 0
        return ((torch.initial_seed() + 0x9E3779B9 * rank) * 1000003
                + self._seed_ctr * seed_stride(self.num_layer)) & 0x7FFFFFFFFFFFFFFF

    # ------------------------------------------------------------------------------------------
    # the hot path: tokens -> logits                 network.py:37-39 + layers.py:223-233,152-161
    # ------------------------------------------------------------------------------------------
    def _bucket_hooks(self, training: bool):
        """name -> the callback that tells the data-parallel wrapper that a gradient bucket is complete (None outside it)"""
        dp = self._dp
        return ((lambda name: (lambda: dp.bucket_ready(name))) if (dp is not None and (dp.world > 1 or dp.force) and training)
                else (lambda name: None))

    def _hidden(self, x: torch.Tensor, wsink: Optional[list] = None) -> torch.Tensor:
        """everything up to the last LayerNorm: tokens [B, L] -> bf16 [B, Lp, d], Lp = L rounded up to the kernels' 32-key tile
        (rows >= L belong to trailing pad tokens)"""
        st = self.store()
        st.sync_shadow()
        training = self.training and torch.is_grad_enabled()
        if training:
            st.attach_grads()
        B, L = x.shape
        if L < 1 or L > self.max_seq:
            raise ValueError(f"sequence length {L} must be in 1 .. max_seq={self.max_seq}")
        tok = x.to(torch.int32).contiguous()
        # The kernels sweep 32-key tiles.  Any other length (the reference takes every L <= max_seq, layers.py:64-109) is
        # right-padded with pad tokens up to the next multiple of 32: trailing pads are masked keys and lie in the causal future
        # of every real position, so the real rows' logits are the reference's; the padded rows are sliced off below and carry
        # no gradient.
        Lp = (L + 31) // 32 * 32
        if Lp != L:
            tok = torch.cat([tok, torch.full((B, Lp - L), self.pad_token, dtype=torch.int32, device=tok.device)], 1)
        d = self.embedding_dim
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed()
        done = self._bucket_hooks(training)

        if self._pad_flag is None or self._pad_flag.device != tok.device:
            self._pad_flag = torch.zeros(1, dtype=torch.int32, device=tok.device)
        padbits = ops.pad_bitmap(tok, self.pad_token, self._pad_flag)
        pe = self.Decoder.pos_encoding.table()
        layer_params = self._layer_params()
        if Lp > self.max_seq:
            # max_seq itself is not a multiple of 32 and L reaches into its last partial tile: the padded rows would index the
            # positional table and the relative embedding beyond max_seq.  Both get zero rows there (E at the FRONT: distance
            # delta reads E[M - 1 - delta], and only padded queries have delta >= max_seq); the padded rows' dE is exactly zero
            # (their dO is), the real rows' is folded back into the layer's gradient slot when the block's backward has run.
            extra = Lp - self.max_seq
            pe = torch.cat([pe, torch.zeros(extra, d, dtype=pe.dtype, device=pe.device)], 0)
            layer_params, done = self._params_for_padded_E(layer_params, extra, done, training)
        P = st.params
        h = ops.embed_pe(tok, P["Decoder.embedding.weight"], pe, p, seed, st.g("Decoder.embedding.weight"),
                         done("embedding"))
        for i, lp in enumerate(layer_params):
            # the layer's gradient bucket is complete when the block's backward (ending in the QKV projection) has run
            h = ops.encoder_layer(h, lp, padbits, p, seed + 4 * i, done(f"layer{i}"), wsink)
        if wsink is not None and Lp != L:
            wsink[:] = [w_[:, :, :L, :L] for w_ in wsink]
        return h

    def _logits_padded(self, x: torch.Tensor, wsink: Optional[list] = None) -> torch.Tensor:
        """the vocabulary projection of ``_hidden``: the whole bf16 [B, Lp, Vp] storage; columns >= V are exact zeros (zero
        weight rows, zero bias)"""
        h = self._hidden(x, wsink)
        st, d, Vp = self.store(), self.embedding_dim, self.vocab_padded
        done = self._bucket_hooks(self.training and torch.is_grad_enabled())
        return ops.linear(h, st.params["fc.weight"], st.padded_view("fc.weight", Vp, d), st.padded_view("fc.bias", Vp, None, "param"),
                          0, st.padded_view("fc.weight", Vp, d, "grad"), st.padded_view("fc.bias", Vp, None, "grad"),
                          done("fc"))

    def _logits(self, x: torch.Tensor, wsink: Optional[list] = None) -> torch.Tensor:
        # [B, Lp, Vp] storage, [B, L, V] view
        return self._logits_padded(x, wsink)[:, : x.shape[1], : self.vocab_size]

    def _params_for_padded_E(self, layer_params, extra, done, training):
        """per-layer operand sets whose relative embedding has `extra` zero rows in front (see _logits), and a bucket callback
        that first folds the temporary dE back into the layer's gradient slot"""
        out, folds = [], {}
        for i, lp in enumerate(layer_params):
            q = ops.LayerParams()
            for k in ops.LayerParams.__slots__:
                setattr(q, k, getattr(lp, k))
            q.E = torch.cat([torch.zeros(extra, 64, dtype=lp.E.dtype, device=lp.E.device), lp.E], 0).contiguous()
            if training:
                q.gE = torch.zeros(q.E.shape, dtype=torch.float32, device=lp.E.device)

                def fold(tmp=q.gE, slot=lp.gE):
                    tmp.record_stream(torch.cuda.current_stream())      # (the bucket callback may run on the side stream of ops.configure_streams)
                    slot.add_(tmp[extra:])
                folds[f"layer{i}"] = fold
            out.append(q)

        def done2(name):
            inner, fold = done(name), folds.get(name)
            if fold is None:
                return inner

            def both():
                fold()
                if inner is not None:
                    inner()
            return both
        return out, done2

    def _layer_params(self):
        """per-layer kernel operands as views of the flat buffers (rebuilt when the store is)"""
        st = self.store()
        if getattr(self, "_lp_store", None) is st:
            return self._lp
        d, P, out = self.embedding_dim, st.params, []
        for i in range(self.num_layer):
            pre = f"Decoder.enc_layers.{i}."
            lp = ops.LayerParams()
            lp.wqkv = st.fused(pre + "rga.Wq.weight", pre + "rga.Wv.weight", 3 * d, d)
            lp.gqkv = st.fused(pre + "rga.Wq.weight", pre + "rga.Wv.weight", 3 * d, d, "grad")
            lp.bqkv = st.fused(pre + "rga.Wq.bias", pre + "rga.Wv.bias", 1, 3 * d, "param").view(3 * d)
            lp.gbqkv = st.fused(pre + "rga.Wq.bias", pre + "rga.Wv.bias", 1, 3 * d, "grad").view(3 * d)
            lp.E, lp.gE = st.w(pre + "rga.E"), st.g(pre + "rga.E")
            # the bias gradients of `fc` and `FFN_suf` are column sums of the LayerNorm backward's dx: that
            # kernel emits them
            lp.wfc, lp.bfc = st.w(pre + "rga.fc.weight"), P[pre + "rga.fc.bias"].data
            lp.gwfc, lp.gbfc = st.g(pre + "rga.fc.weight"), st.g(pre + "rga.fc.bias")
            lp.g1, lp.b1 = P[pre + "layernorm1.weight"].data, P[pre + "layernorm1.bias"].data
            lp.gg1, lp.gb1 = st.g(pre + "layernorm1.weight"), st.g(pre + "layernorm1.bias")
            H, Hp = d // 2, self.ffn_padded
            if Hp == H:
                lp.wpre, lp.bpre = st.w(pre + "FFN_pre.weight"), P[pre + "FFN_pre.bias"].data
                lp.gwpre, lp.gbpre = st.g(pre + "FFN_pre.weight"), st.g(pre + "FFN_pre.bias")
                lp.wsuf, lp.gwsuf = st.w(pre + "FFN_suf.weight"), st.g(pre + "FFN_suf.weight")
            else:           # d = 64 * odd: the kernels see the zero-padded width (FlatStore: padded rows / colpad columns)
                lp.wpre, lp.bpre = st.padded_view(pre + "FFN_pre.weight", Hp, d), st.padded_view(pre + "FFN_pre.bias", Hp, None, "param")
                lp.gwpre, lp.gbpre = st.padded_view(pre + "FFN_pre.weight", Hp, d, "grad"), st.padded_view(pre + "FFN_pre.bias", Hp, None, "grad")
                lp.wsuf, lp.gwsuf = st.padded_view(pre + "FFN_suf.weight", d, Hp), st.padded_view(pre + "FFN_suf.weight", d, Hp, "grad")
            lp.bsuf, lp.gbsuf = P[pre + "FFN_suf.bias"].data, st.g(pre + "FFN_suf.bias")
            lp.g2, lp.b2 = P[pre + "layernorm2.weight"].data, P[pre + "layernorm2.bias"].data
            lp.gg2, lp.gb2 = st.g(pre + "layernorm2.weight"), st.g(pre + "layernorm2.bias")
            out.append(lp)
        self._lp_store, self._lp = st, out
        return out

    def check_no_leading_pads(self) -> None:
        """The library-boundary twin of ``utils.check_no_leading_pads``: every ``forward`` lets the bitmap kernel record, on the
        device, whether some row STARTED with padding and held real tokens later (rows with fully masked queries, outside the
        parity contract with the reference; trailing and interior pads are masked like the reference
        masks them and are accepted).  Reading the record is a device synchronisation, so it is done here, on request --
        train.py calls it where it prints metrics, bench.py after its timed region -- and not inside ``forward``.  Raises
        ValueError and clears the record."""
        if self._pad_flag is not None and int(self._pad_flag.item()) != 0:
            self._pad_flag.zero_()
            raise ValueError(f"a batch handed to MusicTransformer.forward had a row that starts with padding token {self.pad_token} "
                             "and holds real tokens later: leading padding is outside the parity contract with the reference "
                             "(fully masked queries); pads may trail or sit inside a sequence")

    check_pads_trail = check_no_leading_pads      # the name of rounds 4-5

    def forward(self, x, length=None, writer=None):
        if self.training or not self.infer:
            if self.training:
                return self._logits(x)
            # eval: (logits, [attention_weights per layer]) as network.py:40.  The [B,h,L,L] fp32 weights are a
            # debug output (268 MB per layer at cfg2, B=2): they are materialised only on request.
            ws = [] if self.return_attention_weights else None
            logits = self._logits(x, ws)
            return logits, (ws if ws is not None else [])
        return self.generate(x, length, None).contiguous().tolist()

    # ------------------------------------------------------------------------------------------
    # sampling                                                                   network.py:44-80
    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _logits_nomask(self, window: torch.Tensor) -> torch.Tensor:
        """logits [B,W,V] of ``Decoder(window, mask=None)`` + fc -- the reference's sampling call (network.py:60-63): every
        position attends to every position of the window, the relative term only reaches back (j <= i).  The window is
        right-padded to the kernels' multiple of 32; the padding rows are excluded as keys (Lk = W) and dropped as queries."""
        st = self.store()
        st.sync_shadow()
        B, W = window.shape
        Lp = (W + 31) // 32 * 32
        if W > self.max_seq:
            raise ValueError(f"window {W} > max_seq={self.max_seq}")
        dev, d, Pm = st.param.device, self.embedding_dim, st.params
        seq = torch.zeros(B, Lp, dtype=torch.int32, device=dev)
        seq[:, :W] = window.to(torch.int32)
        pe, layer_params = self.Decoder.pos_encoding.table(), self._layer_params()
        if Lp > self.max_seq:          # max_seq is no multiple of 32: zero rows for the padded positions (see _logits)
            pe = torch.cat([pe, torch.zeros(Lp - self.max_seq, d, dtype=pe.dtype, device=pe.device)], 0)
            layer_params, _ = self._params_for_padded_E(layer_params, Lp - self.max_seq, lambda name: None, False)
        hh = ops.embed_pe_fwd(seq, Pm["Decoder.embedding.weight"].data, pe)
        for lp in layer_params:
            qkv = ops.linear_fwd(hh, lp.wqkv, lp.bqkv, 0)
            att = ops.rel_attn_fwd_nomask(qkv, lp.E, W)
            o1 = ops.add_ln_fwd(ops.linear_fwd(att, lp.wfc, lp.bfc, 0), hh, lp.g1, lp.b1, 1e-6)[0]
            f = ops.linear_fwd(ops.linear_fwd(o1, lp.wpre, lp.bpre, 1), lp.wsuf, lp.bsuf, 0)
            hh = ops.add_ln_fwd(f, o1, lp.g2, lp.b2, 1e-6)[0]
        Vp = self.vocab_padded
        logits = ops.linear_fwd(hh, st.padded_view("fc.weight", Vp, d), st.padded_view("fc.bias", Vp, None, "param"), 0)
        return logits[:, :W, : self.vocab_size]

    @torch.no_grad()
    def next_token_probs(self, window: torch.Tensor, reference_mask: bool = False) -> torch.Tensor:
        """softmax of the logits that follow the last token of ``window`` [B,W].  Default: causal semantics (the
        training-time mask, see DESIGN.md 'decode semantics'); windows that are no multiple of 32 are right-padded inside
        ``_logits`` with pad tokens, which lie in the masked future of every real position.  ``reference_mask=True``: the reference's own
        sampling call, ``Decoder(window, mask=None)`` (network.py:60-62)."""
        B, W = window.shape
        if reference_mask:
            return torch.softmax(self._logits_nomask(window)[:, W - 1].float(), -1)
        was = self.training                   # (_logits pads the window to the kernels' 32-key tile itself)
        self.eval()
        logits = self._logits(window)[:, W - 1].float()
        self.train(was)
        return torch.softmax(logits, -1)

    @torch.no_grad()
    def generate(self, prior: torch.Tensor, length=2048, tf_board_writer=None, temperature: float = 1.0,
                 top_k: int = 0, top_p: float = 1.0, reference_mask: bool = False):
        """Autoregressive sampling with the reference's sliding window (config.threshold_len) and
        full-softmax categorical sampling by default (top_k=0, top_p=1.0 == the reference's
        OneHotCategorical, network.py:73-74); top-k / top-p / temperature are opt-in extras.
        ``reference_mask=True`` reproduces the reference's step exactly -- ``Decoder(decode_array, None)``, i.e. NO look-ahead
        mask at sampling time (network.py:60) -- instead of the training-time causal semantics."""
        decode_array = prior
        result_array = prior
        for _ in range(length):
            if decode_array.size(1) >= config.threshold_len:
                decode_array = decode_array[:, 1:]
            probs = self.next_token_probs(decode_array, reference_mask)
            probs = filter_probs(probs, temperature, top_k, top_p)
            nxt = torch.multinomial(probs, 1).to(decode_array.dtype)
            decode_array = torch.cat((decode_array, nxt), dim=-1)
            result_array = torch.cat((result_array, nxt), dim=-1)
        return result_array

    # KV-cache decode (cfg5): O(t) per token instead of the reference's O(W^2) recompute; the driver is decode.py
    @torch.no_grad()
    def generate_cached(self, prior: torch.Tensor, length: int, temperature: float = 1.0, top_k: int = 0,
                        top_p: float = 1.0, seed: int = 0, use_graph: bool = True, return_probs: bool = False,
                        grammar=None, prefill: str = "auto", return_cache: bool = False, groups: Optional[int] = None,
                        masked_groups: bool = False, prior_lengths=None, kv_cache: str = "bf16", window: Optional[int] = None,
                        hop: Optional[int] = None, samples_per_prompt: Optional[int] = None, note_rules=None,
                        max_polyphony: Optional[int] = None, repetition=None, lookahead: Optional[int] = None,
                        draft="history", draft_ngram: int = 3, stats: Optional[dict] = None, class_sampling=None,
                        entropy_sampling=None):
        """Sample ``length`` events after ``prior`` [B,P] with per-layer K/V caches and absolute positions
        0..P+length-1 (requires P+length <= max_seq unless ``window`` is given, see below).  Every step runs
        embed -> N x (QKV GEMM, cached relative attention, fc, LN, FFN, LN) -> vocabulary GEMM -> fused
        sampler; the position lives on the device, so after a warm-up step the whole step is captured in
        one graph and replayed per token.  Returns int32 [B, P+length] (and, if ``return_probs``, the
        f32 [B, P+length, V] next-token distributions, position p = distribution after token p).
        ``prefill``: "batched" runs the first P-1 prior tokens through the full-sequence (training) kernels in ONE pass and
        copies every layer's K/V rows into the caches -- a 500-event prompt costs one forward instead of 499 decode steps;
        "token" teacher-forces the prior step by step; "auto" = batched for priors of more than 32 tokens (not with
        ``return_probs``, which wants the distribution after every prior token; falls back to "token" when the prompt padded
        to a multiple of 32 rows would exceed max_seq).  The two prefill paths fill the caches through different GEMM kernels
        (same values to bf16 rounding, not bitwise), so with a fixed seed the SAMPLED continuation may differ between a
        33-token and a 32-token prompt's path: pass ``prefill`` explicitly where run-to-run identical samples matter.
        ``return_cache`` adds the per-layer (K, V) caches to the result (parity tests).

        ``prior_lengths`` (length-B ints): prompts of different lengths P_b, right-padded into ``prior`` [B, Pmax] (entries at or
        beyond P_b are ignored).  One batched causal prefill covers prior[:, :Pmax-1] (a row's cache rows past P_b-2 are
        overwritten by its own decode steps before they are read), then every row decodes ``length`` tokens in lockstep from
        its own position P_b-1 (per-row positions on the device, the kernels' per_row; graph capture, ``groups`` and ``grammar``
        as above).  Returns int32 [B, Pmax+length]: row b holds its prompt, its ``length`` sampled tokens, then ``pad_token``.
        Unequal lengths need the batched prefill ("token" is refused; "auto" means "batched").  With ``return_probs`` row b
        carries the distributions after positions P_b-1 .. P_b+length-2 and zeros elsewhere -- unlike the uniform case, which
        prefills token by token to report every position.  With ``return_cache`` row b's cache rows from P_b+length-1 on
        are zero, as the uniform case leaves its rows from P+length-1 on.  All lengths equal: exactly the call without
        ``prior_lengths`` on prior[:, :P] (bitwise), its outputs padded to Pmax+length as above.

        ``kv_cache``: "bf16" (default) or "fp8", an opt-in 8-bit cache -- OCP e4m3fn codes with one f32 scale per (b, h, row)
        (format: include/mgx.h, ABI 20) -- that streams 136 instead of 256 bytes per key and (b, h) and holds a batch in 53 % of
        the memory.  Every K / V row is quantized as it enters the cache (the batched prefill through ops.kv_store_fp8), so the
        distributions and samples differ from the bf16 run.  Works with every option above; with
        ``return_cache`` the result is (res, K codes, V codes, K scales, V scales) per layer, the codes as float8_e4m3fn
        [B, h, L, 64] and the scales f32 [B, h, L].

        ``window`` (2 .. max_seq) and ``hop`` (default max(1, window // 8)): generate past max_seq.  The cache holds a window of
        at most ``window`` tokens of every row, numbered from position 0 (the model's positional encoding is absolute, so a
        cache cannot slide by one token: every cached row would belong to the wrong position).  Row b keeps on the device the
        output column ``base_b`` of its window position 0 and the window position ``t_b`` of the step's input token; a prompt
        longer than the window starts from its last ``window`` tokens.  Whenever the longest row has filled the window
        (max_b t_b == window) every row is re-anchored: the oldest ``hop`` tokens are dropped (t_b -= hop, base_b += hop), the
        rest renumbered from 0 and their K / V rebuilt by one batched causal pass of window - hop rows (the prefill, for either
        ``kv_cache``); the sampler draws by the absolute step base_b + t_b, so segments do not repeat random numbers.  Each
        step's distribution is the causal forward of the tokens out[b, base_b : base_b + t_b + 1]: with hop = 1 the window of
        ``generate`` (whose forward sees config.threshold_len - 1 tokens: ``window`` = 499), with a larger hop a window
        of between window - hop + 1 and window tokens at one forward pass per hop tokens.  ``decode.window_schedule`` gives the whole
        schedule on the host; nothing is read back and the step graph is captured once and replayed across re-anchors.
        ``prior.shape[1] + length`` may exceed max_seq; the prefill is always batched ("token" is refused, as are ``groups`` and
        ``masked_groups``), ``hop`` + the spread of the rows' start positions must stay below ``window``, and
        window - hop rounded up to 32 rows must fit max_seq.  Returns int32 [B, Pmax+length] as above; with ``return_probs``
        row b carries the distributions after columns P_b-1 .. P_b+length-2 and zeros elsewhere (uniform prompts too); with
        ``return_cache`` the last window's caches, min(window, Pmax+length) rows, zero beyond the row of each row's last input
        token.  While no re-anchor happens (window >= Pmax + length) tokens, distributions and caches are bitwise those of the
        call without ``window`` and with the batched prefill.

        ``samples_per_prompt`` (N, 1 .. 16): N continuations of every prompt over ONE copy of its K/V.  ``prior`` [Bp, P] (with
        ``prior_lengths``, or all of width P) gives int32 [Bp * N, Pmax+length], row b * N + n the n-th sample of prompt b, padded
        as the ragged call pads; with ``return_probs`` the f32 [Bp * N, Pmax+length, V] distributions after positions
        P_b-1 .. P_b+length-2 of every row.  One batched prefill of the Bp prompts fills a prompt cache that the decode never
        writes; every row appends to a cache of its own of ``length`` rows, and the attention (mgx_rel_attn_decode_shared,
        ABI 26) loads a prompt's keys once for the samples of that prompt.  Row r draws with (seed, position, r), as it does in
        the call on ``prior.repeat_interleave(N, 0)``; the two calls run different kernels, so their distributions agree to
        rounding and a draw near a CDF boundary may differ.  Prefill work and prompt-cache memory are 1/N of the repeated
        call's.  Refused: ``window``, ``kv_cache="fp8"``, ``groups`` > 1, ``masked_groups``, ``prefill="token"``,
        ``return_cache``, Pmax + length > max_seq.  None (default): the call as described above, untouched.

        ``note_rules`` (integers [vocab_size], ``EventSeq.note_rules(vocab_size)`` for the MIDI-like codec) and
        ``max_polyphony`` (1 .. 128, None: no cap): well-formed note streams.  rule[v] = +(k+1): id v turns key k on,
        -(k+1): it turns key k off, 0: neither.  Every row keeps on the device the set of keys it holds (include/mgx.h, ABI
        28), starting from what its own prompt leaves held (folded on the host: a key is held iff the last prompt id that
        touched it turned it on -- the prompt may be ill-formed or above the cap).  Before the sampler every note_on of a held
        key, every note_off of a silent key and, once ``max_polyphony`` keys are held, every note_on is masked out of the logits
        (mgx_notes_mask; so also out of ``return_probs`` and under top-k / top-p), and after it the draw is applied to the
        row's set (mgx_notes_account); the launches are captured with the step.  A row is the unconstrained row of the same
        seed up to the first step at which that one breaks a rule: the step also draws once BEFORE the mask, with ``seed``,
        and a legal first draw stands (mgx_notes_keep); the masked draw uses a seed of its own, so without top-k / top-p the
        token has exactly the masked distribution.  Works with ``prior_lengths``, ``kv_cache``, ``window``,
        ``return_probs``, ``use_graph``, ``prefill`` ("token": the teacher-forced prompt steps are not constrained) and
        ``samples_per_prompt``; the return values do not change (``EventSeq.held_after(row)`` gives a row's final held keys).
        Refused (ValueError, before any device work): ``max_polyphony`` without ``note_rules`` or outside 1 .. 128; rules that
        are not integers [vocab_size], exceed +-128, are not 0 at pad_token, or name a key with only one of its two ids (with
        these the mask can never leave a row without an allowed id); ``grammar`` (the two masks together could), ``groups`` > 1,
        ``masked_groups``, ``return_cache``.  None (default): the call as described above, untouched.

        ``repetition`` (a ``decode.Repetition(subject, presence, frequency, window, ngram, span, ban)``): repetition control.
        Before the sampler (and before the first draw of ``note_rules``) one stateless launch per step, captured with it
        (mgx_repeat_penalty, ABI 31), reads the row's own history -- its columns of the token matrix, the prompt included --
        and subtracts ``presence + frequency * c`` from the logit of every id v with ``subject[v] != 0`` that occurs c > 0 times
        among the row's last ``window`` tokens, and ``ban`` (default 1e4) from every id that would complete an ``ngram``-gram
        the row holds already within its last ``span`` tokens (0: the whole sequence so far).  ``EventSeq.repeat_subject()``
        names the note_on ids, the musical default.  The amounts are finite: the set of finite logits does not change, so it
        works unchanged with ``grammar``, ``note_rules``, ``generate_timed``'s budgets, ``prior_lengths``, ``kv_cache``,
        ``window`` / ``hop`` (the history is in absolute columns), ``samples_per_prompt`` and ``return_cache``, and where the
        other masks leave only a banned id, that id is drawn.  With ``return_probs`` the distributions are those of the
        PENALISED logits.  Teacher-forced ``prefill="token"`` prompt steps stay unpenalised.  Refused (ValueError, before any
        device work): a ``subject`` that is not integers [vocab_size] or not 0 at pad_token; ``presence`` / ``frequency``
        negative or not finite; ``window`` outside 1 .. 4096; ``ngram`` not 0 or 2 .. 64; ``span`` not 0 or >= ``ngram``; ``ban``
        outside (0, 1e4]; presence + frequency * window > 1e4; ``groups`` > 1, ``masked_groups``.  None (default), or an
        object with no penalty and no n-gram rule: the call as described above, untouched, with no new launch.

        ``lookahead`` (T, 2 .. 8), ``draft`` ("history" or a guide) and ``draft_ngram`` (1 .. 8, default 3): draft and verify,
        several tokens per step with the same sample.  Both bounds of a step -- its ~40 launches and one pass over the row's
        K/V -- are paid per step, not per token, and music repeats its own figures.  A step guesses the row's next T - 1
        tokens (mgx_lookahead_draft, ABI 32): with "history" the continuation of the latest earlier occurrence of the row's
        last ``draft_ngram`` tokens in its own sequence (then of fewer, down to one; extended periodically where the match runs
        into the present; pad_token without a match), with a guide -- integers [B, >= Pmax], e.g. an earlier result -- its
        columns.  The T positions t_b .. t_b + T - 1 of every row then run as B * T rows of the ordinary step on the guessed
        inputs, the attention (mgx_rel_attn_decode_multi) loading every K / V row once for the T queries, and
        mgx_lookahead_accept draws every position with the draw the one-token call makes there -- the sampler's draw is a
        pure function of (seed, column, row), so no rejection-sampling arithmetic -- and keeps the prefix whose guesses were
        right: 1 to T tokens per step and row.  The result is the one-token call's sample for that seed up to the rounding
        difference between the two chains' kernels (a last-bit difference may flip a draw near a CDF boundary).  Nothing is
        rolled back: cache rows of rejected guesses lie above the row's new position and are rewritten before they are read.
        The step is captured once and replayed in runs of 32; between runs the host reads the rows' done flags and stops when
        every row holds its last token, after at most ``length`` steps.  Returns what the call without it returns, padded as
        the ragged call pads; with ``return_probs`` row b carries the distributions after columns P_b-1 .. P_b+length-2 and
        zeros elsewhere (uniform prompts too; the prompt is always prefilled in one batched pass).  ``stats`` (a dict)
        receives ``steps`` and ``tokens``, one int per row, and ``steps_run``.  Works with ``prior_lengths``, ``grammar`` (the
        grammar row of position i is that of draft token i), ``return_probs``, ``use_graph`` and ``seed``.  Refused
        (ValueError, before any device work), all of them later work: T outside 2 .. 8, ``draft_ngram`` outside 1 .. 8, a
        guide that is not integers [B, >= Pmax]; ``window`` / ``hop``, ``kv_cache="fp8"``, ``samples_per_prompt``, ``groups`` > 1,
        ``masked_groups``, ``prefill="token"``, ``return_cache``; ``note_rules``, ``max_polyphony`` and ``repetition``, whose
        state is sequential (position i + 1 depends on the token at i); ``generate_timed`` and ``generate_beam`` refuse the
        keyword.  None (default): the call as described above, untouched, with no new launch.

        ``class_sampling`` (a ``decode.ClassSampling(classes, temperature, top_k, top_p)``): a temperature, a top-k and a top-p
        per class of ids -- steadier rhythm with freer pitches, velocities from the top few, chords from a nucleus.
        ``classes`` (integers [vocab_size], classes 0 .. 15) comes from the codec: ``EventSeq.event_classes(vocab_size)``
        gives the names and the array.  Sampling is in two stages: the class is drawn with the model's own probability at the
        call's ``temperature`` (no mass moves between classes), the id inside class c from the softmax at ``temperature[c]`` cut
        by ``top_k[c]`` and ``top_p[c]`` with the sampler's rules (ties stay together; the grammar's ids only).  One stateless
        launch per step, captured with it (mgx_class_logits, ABI 33), writes bf16(ln p') of that distribution over the step's
        logits -- after the budget's mask and the repetition penalty -- and the unchanged sampler then runs at temperature 1
        with the call's own ``top_k`` / ``top_p``, which act on p' as a whole.  ``return_probs`` files softmax(bf16(ln p')), what
        was drawn from: a probability is off by at most |ln p'| 2^-8 relative, the order of the bf16 logits themselves.  Works
        with ``prior_lengths``, ``kv_cache``, ``window`` / ``hop``, ``samples_per_prompt``, ``grammar``, ``repetition``,
        ``generate_timed`` and ``lookahead`` (row-wise and stateless); teacher-forced ``prefill="token"`` prompt steps stay
        unwarped.  Refused (ValueError, before any device work): ``classes`` that are not integers [vocab_size] in 0 .. 15; a
        temperature that is not finite and > 0 (the call's included); a ``top_k`` that is not an integer >= 0; a ``top_p``
        outside (0, 1]; a sequence that is not one value per class; ``groups`` > 1, ``masked_groups``; ``note_rules`` /
        ``max_polyphony`` (that step draws twice and an in-place rewrite cannot serve both: later work).  ``generate_beam``,
        ``generate`` and ``Event_Melody_RNN`` do not take the keyword.  None (default), or an object whose every class has the
        call's temperature and no filter: the call as described above, untouched, with no new launch.

        ``entropy_sampling`` (a ``decode.EntropySampling(min_p, typical_p, tau, eta, trace)``): three cuts that follow the row's
        own uncertainty, where ``top_k`` / ``top_p`` keep the same share whether the model is certain or lost.  ``min_p`` keeps
        the ids with at least that share of the most likely id's probability; ``typical_p`` keeps the ids whose surprise lies
        closest to the row's entropy, up to that mass (locally typical sampling); ``tau`` is Mirostat v2, a feedback loop per row
        that holds the surprise of what is drawn near ``tau`` bits -- ids more surprising than the row's threshold mu are cut
        (the most likely ids stand in where that leaves none), mu starts at 2 tau and moves by -eta (surprise - tau) after every
        draw.  The stages run in that order, each on the survivors of the one before, as a pure mask: one launch per step, the
        last before the sampler (mgx_entropy_mask, ABI 34; after the budget's mask, the penalty and ``class_sampling``), writes
        -inf and nothing else, so the unchanged sampler runs at the call's ``temperature`` (1 after ``class_sampling``) with its
        own ``top_k`` / ``top_p`` and ``return_probs`` files the model's distribution renormalised over what was kept.  With
        ``tau`` or ``trace=True`` a second launch after the sampler (mgx_entropy_account) computes the drawn token's surprise under
        the distribution before the mask, moves mu and files the trace.  After the call the object holds the state: ``mu``
        float32 [rows] and, with ``trace``, ``surprise`` float32 [rows, columns], NaN where nothing was generated.  Works with
        ``prior_lengths``, ``kv_cache``, ``window`` / ``hop``, ``samples_per_prompt`` (a threshold per sample), ``grammar``,
        ``repetition``, ``class_sampling`` and ``generate_timed``; under ``lookahead`` only the stateless part works, ``min_p``
        and ``typical_p`` on the B * T rows.  Refused (ValueError, before any device work): ``min_p`` outside [0, 1),
        ``typical_p`` outside (0, 1], a ``tau`` that is not finite and > 0, ``eta`` outside (0, 1]; ``tau`` / ``trace`` with
        ``lookahead`` (the state is sequential: later work); ``note_rules`` / ``max_polyphony`` (that step draws twice: later
        work); ``groups`` > 1, ``masked_groups`` (later work).  ``generate_beam``, ``generate`` and ``Event_Melody_RNN`` do not
        take the keyword.  None (default), or an object with min_p 0, typical_p 1, no tau and no trace: the call as described
        above, untouched, with no new launch."""
        return decode.generate_cached(self, prior, length, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                                      use_graph=use_graph, return_probs=return_probs, grammar=grammar, prefill=prefill,
                                      return_cache=return_cache, groups=groups, masked_groups=masked_groups,
                                      prior_lengths=prior_lengths, kv_cache=kv_cache, window=window, hop=hop,
                                      samples_per_prompt=samples_per_prompt, lookahead=lookahead, draft=draft,
                                      draft_ngram=draft_ngram, stats=stats, note_rules=note_rules, max_polyphony=max_polyphony,
                                      repetition=repetition, class_sampling=class_sampling, entropy_sampling=entropy_sampling)

    @torch.no_grad()
    def generate_timed(self, prior: torch.Tensor, budget, cost, max_length: int, *, inclusive: bool = True, poll: int = 32,
                       temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, use_graph: bool = True,
                       grammar=None, prior_lengths=None, kv_cache: str = "bf16", window: Optional[int] = None,
                       hop: Optional[int] = None, return_probs: bool = False, note_rules=None,
                       max_polyphony: Optional[int] = None, repetition=None, class_sampling=None, entropy_sampling=None,
                       **refused):
        """Generate to a musical length: ``generate_cached`` where every row stops at a budget of its own instead of after a
        number of events.  ``cost`` (int32-representable [vocab_size], >= 0, 0 at pad_token) prices every id --
        ``EventSeq.time_cost`` in centiseconds, ``REMI_EventSeq.bar_cost`` in bars -- and ``budget`` (an int, or one per row;
        None = no budget) is what a row's CONTINUATION may cost; ``max_length`` caps its events.  A budget of 0 generates
        nothing.  Each row keeps its clock on the device (include/mgx.h, ABI 27): before the sampler every id that costs more
        than the row has left is masked out of the logits (mgx_budget_mask), so no row overshoots -- also under top-k / top-p
        and ``grammar`` -- and after it the draw is charged (mgx_budget_account) and a row whose budget is spent ends.
        ``inclusive=True``: the token that spends the last unit stays, so the row lands exactly on its budget (seconds);
        ``inclusive=False``: that token is dropped -- the N-th new ``bar`` closes bar N and is not part of it.  An ended row
        goes on stepping on pad tokens beside the others (positions never stop), and after every ``poll`` steps the host reads
        the rows' flags once -- the only synchronisation -- and stops when all have ended, so the call costs the steps of its
        longest row rounded up to ``poll``, not ``max_length``.  (A row with only a few units left waits for an id cheap
        enough -- a short time shift -- and may reach ``max_length`` first: it then has spent less than its budget.)  The other arguments are ``generate_cached``'s (prefill "auto").
        Returns (tokens int32 [B, Pmax+max_length]: prompt, kept events, then pad_token;  lengths int32 [B]: the events every
        row kept;  info: ``steps_run``, ``spent`` int64 [B] (the cost of the kept events), ``remaining`` and ``done`` [B] as the
        device left them, and ``probs`` f32 [B, Pmax+max_length, V] with ``return_probs`` -- the distributions the sampler saw,
        0 at every masked id).  Refused (ValueError, before any device work): ``samples_per_prompt``, ``groups`` > 1,
        ``masked_groups``, ``return_cache``, ``beam_size``, ``lookahead`` (other drivers), a malformed ``cost``, ``poll`` < 1, ``budget`` < 0,
        ``max_length`` < 1, and what ``generate_cached`` refuses.  ``note_rules`` / ``max_polyphony``: as in
        ``generate_cached`` -- the budget's mask and account run first, the notes' second; an ended row steps on pad_token,
        whose rule is 0, so its held set stays what it was when the row ended.  ``repetition``: as in ``generate_cached`` --
        after the budget's mask, before the notes' first draw; ``probs`` are then those of the penalised logits.
        ``class_sampling``: as in ``generate_cached`` -- after the budget's mask and the penalty; a masked id stays masked, so
        no row overshoots; ``probs`` are then softmax(bf16(ln p')).
        ``entropy_sampling``: as in ``generate_cached`` -- the last mask before the sampler, and its account runs before the
        budget's, which may replace the token by a pad; the trace of an ended row is NaN from its end on."""
        return decode.generate_timed(self, prior, budget, cost, max_length, inclusive=inclusive, poll=poll, temperature=temperature,
                                     top_k=top_k, top_p=top_p, seed=seed, use_graph=use_graph, grammar=grammar,
                                     prior_lengths=prior_lengths, kv_cache=kv_cache, window=window, hop=hop,
                                     return_probs=return_probs, refused=refused, note_rules=note_rules,
                                     max_polyphony=max_polyphony, repetition=repetition, class_sampling=class_sampling,
                                     entropy_sampling=entropy_sampling)

    @torch.no_grad()
    def generate_beam(self, prior: torch.Tensor, length: int, beam_size: int, temperature: float = 1.0, stochastic: bool = False,
                      seed: int = 0, grammar=None, prior_lengths=None, kv_cache: str = "bf16", use_graph: bool = True,
                      return_beams: bool = False, note_rules=None, max_polyphony: Optional[int] = None, lookahead=None):
        """Beam search over the KV-cache decode: the ``beam_size`` (K, 1 .. min(16, V)) best continuations of ``length`` events
        of every prompt of ``prior`` [B,P], each prompt searched with its own beam.  A beam's score is the sum of its events'
        log softmax(logits / temperature) (under ``grammar``: over the allowed events, the sampler's rule).  The search starts
        from ONE live beam per prompt (the others at -inf, as ``Event_Melody_RNN.beam_search``); every step runs the decode
        chain on the B * K rows, keeps the K best of the K * V expansions on the device (mgx_beam_select; exact ties go to the
        smaller k * V + v) and hands every survivor its parent's cache rows (mgx_kv_beam_reorder, between two caches), so the
        step is graph-captured -- two steps per graph -- and nothing is read back.  ``stochastic``: survivors are chosen by
        Gumbel-perturbed scores, a pure function of (``seed``, position, row, event); the scores carried and returned stay the
        unperturbed sums.  With fewer than K finite candidates (a grammar that allows fewer) the spare beams are dead: score
        -inf, their tokens copies of the best beam's.  ``prior_lengths``, ``kv_cache`` and ``grammar`` as in ``generate_cached``;
        P + length <= max_seq, the prompt is prefilled in one batched pass.  K = 1 is greedy decoding.
        Returns (tokens int32 [B, Pmax+length] of the best beam of every prompt, padded as ``generate_cached`` pads ragged
        rows; scores f32 [B]).  ``return_beams`` appends all beams int32 [B, K, Pmax+length], their scores f32 [B, K] and the
        two history tables int32 [B, K, Pmax+length]: column c of slot j holds the token chosen for that slot at column c and
        the slot (0..K-1) of the previous column that it extends.  ``note_rules`` / ``max_polyphony`` are refused (ValueError): a
        beam's held notes would have to follow its parent through the reorder, which is not built.  ``lookahead`` is refused
        too: draft and verify keeps one sampled sequence per row, a search ranks K * V expansions per step."""
        if lookahead is not None:
            raise ValueError("generate_beam is not combined with lookahead (draft and verify is generate_cached(lookahead=): a "
                             "search has no single draw per position to verify a guess against)")
        if note_rules is not None or max_polyphony is not None:
            raise ValueError("generate_beam is not combined with note_rules / max_polyphony (a beam's held notes would have to "
                             "follow its parent through the reorder: not built)")
        return decode.generate_beam(self, prior, length, beam_size, temperature=temperature, stochastic=stochastic, seed=seed,
                                    grammar=grammar, prior_lengths=prior_lengths, kv_cache=kv_cache, use_graph=use_graph,
                                    return_beams=return_beams)

    @torch.no_grad()
    def score(self, x: torch.Tensor, lengths=None, from_pos=None, temperature: float = 1.0, grammar=None, logits: str = "auto",
              window: Optional[int] = None, stride: Optional[int] = None):
        """The log-probability the model gives to every event of ``x`` [B, L]: ``logp[b, i] = log p(x[b, i] | x[b, :i])`` under
        softmax(logits / temperature).  Runs without gradients and with dropout off whatever ``self.training`` is (the mode is
        restored).  Returns a dict: ``logp`` f32 [B, L]; ``hit`` int32 [B, L] (1: the event is the model's arg-max, the smallest id
        among equal maxima; 0: it is not; -1: unscored); ``sum`` f64 [B], ``count`` and ``hits`` int32 [B], the totals over a row's
        scored events (mgx_score_reduce).

        Event i of row b is scored iff i >= max(1, from_pos[b]), i < lengths[b] (when ``lengths`` is given) and
        x[b, i] != pad_token; everything else is unscored: logp 0, hit -1.  Column 0 never is scored: the model has no start
        token.  ``lengths`` and ``from_pos`` are host integers (one per row; ``from_pos`` may be one for all).

        ``logits``: "fp32" takes the log-sum-exp from the fp32 accumulators of the vocabulary projection and never stores the
        logits (mgx_linear_logprob on ``_hidden``); "bf16" runs ``_logits`` and then mgx_token_logprob on the bf16 logits, as the
        decode path reads them -- ``generate_beam``'s scores are sums of these; "auto" is fp32 unless a ``grammar`` is given or
        d > 1024.  ``grammar``: a ``next_token_table()`` as in ``generate_cached`` (the log-softmax runs over the events that may
        follow x[b, i-1]; a disallowed event scores -inf); refused with "fp32".

        ``window`` (W, 2 .. max_seq; default max_seq) and ``stride`` (1 .. W - 1; default max(1, W // 2)): a row of more than W
        events is scored in overlapping windows (``scoring.score_schedule``), each renumbered from position 0 as a training crop
        is; every event is scored exactly once, outside the first window with at least W - stride events of context.  Rows of
        different lengths are scheduled per row and their windows batched by width; rows that fit W ride in one window.
        A NaN or +inf logit makes the row's entries NaN.  Leading pads follow ``forward``'s rule (``check_no_leading_pads``).
        Nothing is read back: the call makes no host synchronisation."""
        from . import scoring
        was = self.training
        self.eval()
        try:
            return scoring.score(self, x, lengths, from_pos, temperature, grammar, logits, window, stride)
        finally:
            self.train(was)

    def test(self):
        self.eval()
        self.infer = True


def filter_probs(probs: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """temperature / top-k / nucleus filtering of a probability matrix [B,V]; identity at defaults."""
    if temperature != 1.0:
        probs = torch.softmax(torch.log(probs.clamp_min(1e-30)) / temperature, -1)
    if top_k and top_k < probs.shape[-1]:
        kth = probs.topk(top_k, -1).values[:, -1:]
        probs = torch.where(probs >= kth, probs, torch.zeros_like(probs))
    if top_p < 1.0:
        sp, si = probs.sort(-1, descending=True)
        cum = sp.cumsum(-1)
        keep = (cum - sp) < top_p * cum[:, -1:]
        sp = torch.where(keep, sp, torch.zeros_like(sp))
        probs = torch.zeros_like(probs).scatter(-1, si, sp)
    return probs / probs.sum(-1, keepdim=True)
