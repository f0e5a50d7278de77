"""Float64 references and exact expectations for the sentence embedder (csrc/tan_w2v.hip, temporalalignnet_amd/word2vec_model.py), in
plain torch on any device.  tests/test_w2v_fp64_gpu.py runs the kernels and the model against them; tests/test_w2v_cases_cpu.py
checks this file.

The model reference (`operands` + `forward`) is the math of oracle.w2v_ref.forward with two changes:

  operands   read as the kernels read them: in bf16 mode the table rows, fc1.weight and fc2.weight are rounded to bf16 and upcast; the
             biases stay f32; h takes its stored (bf16) value by a straight-through term, so the pooling sees what tan_wordpool_fwd
             sees while the gradient is the unrounded chain's.  Ids outside [0, V) read row 0 (tan_embed_gather).
  pooling    written out with the kernel's rule -- the LOWEST word index among equal maxima (`first_max`) -- instead of
             torch.max(dim), whose tie index is unspecified on a device.  Masked words are filled with -6e4; a sentence whose mask
             is all zero keeps every word (word2vec_model.py:92-93).

Ties are not rare: without an attention mask the trailing id-0 words of a sentence are identical rows, every channel that is 0 after
the ReLU ties over all words, and bf16 rounding merges values closer than 2^-8 relative.

The kernel-level expectations (`gather_expected`, `wordpool_expected`, `wordpool_bwd_expected`) are exact: those kernels select and
copy.  `exact_params` puts the fc1 path on grids where h is exact in f32, so that no selection of the model test hangs on a rounding
error (its docstring has the measurement that made this necessary)."""
import torch

F64 = torch.float64
D_WORD, D_PAD, D_HID, D_OUT = 300, 320, 2048, 512
FILL = -6e4
GRAD_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


# ----------------------------------------------------------------------------------------------------------------------
# the pooling rule
# ----------------------------------------------------------------------------------------------------------------------
def first_max(h, keep=None):
    """h [M, W, H] (float64 for autograd; any float dtype otherwise), keep [M, W] (nonzero = the word takes part) or None
    -> pooled [M, H] float64, first [M, H] int64: the maximum over the words with masked words at -6e4, and the lowest word index
    that attains it.  Differentiable in h (the gradient goes to that one index)."""
    hd = h.to(F64)
    M, W, H = hd.shape
    if keep is not None:
        hd = hd.masked_fill(~keep.bool()[:, :, None], FILL)
    ar = torch.arange(W, device=hd.device)
    first = torch.where(hd == hd.amax(1, keepdim=True), ar[None, :, None], W).amin(1)
    return hd.gather(1, first[:, None, :])[:, 0], first


def last_max(h, keep=None):
    """the same with the HIGHEST index among equal maxima: what flipping `>` to `>=` in the kernel's compare would give"""
    hd = h.to(F64)
    if keep is not None:
        hd = hd.masked_fill(~keep.bool()[:, :, None], FILL)
    ar = torch.arange(hd.shape[1], device=hd.device)
    last = torch.where(hd == hd.amax(1, keepdim=True), ar[None, :, None], -1).amax(1)
    return hd.gather(1, last[:, None, :])[:, 0], last


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def operands(p, bf16, device=None):
    """p: the f32 state dict of Word2VecModel -> float64 tensors as the kernels read them; fc1 / fc2 are leaves that require grad"""
    q = {}
    for k, v in p.items():
        v = torch.as_tensor(v).detach().float()
        if device is not None:
            v = v.to(device)
        if bf16 and k in ("word_embd.weight", "fc1.weight", "fc2.weight"):
            v = v.bfloat16()
        q[k] = v.to(F64).clone().requires_grad_(k != "word_embd.weight")
    return q


def keep_mask(attention_mask):
    """1 = keep; an all-zero row keeps everything"""
    keep = attention_mask.bool()
    return keep | (keep.sum(-1, keepdim=True) == 0)


def forward(q, input_ids, attention_mask=None, bf16=False, pool=first_max):
    """q: `operands`.  -> {'pooler_output' [M, 512], 'last_hidden_state' [M, W, 512], 'h' [M, W, 2048], 'first' [M, 2048]}"""
    V = q["word_embd.weight"].shape[0]
    ids = input_ids.long()
    ids = torch.where((ids < 0) | (ids >= V), torch.zeros_like(ids), ids)
    x = q["word_embd.weight"][ids]
    h = torch.relu(x @ q["fc1.weight"].t() + q["fc1.bias"])
    if bf16:
        h = h + (h.bfloat16().double() - h).detach()
    pooled, first = pool(h, None if attention_mask is None else keep_mask(attention_mask))
    return {"pooler_output": pooled @ q["fc2.weight"].t() + q["fc2.bias"],
            "last_hidden_state": h @ q["fc2.weight"].t() + q["fc2.bias"], "h": h, "first": first}


def forward_backward(p, input_ids, attention_mask, cotangent, bf16=False, device=None, pool=first_max):
    """-> (outputs detached, {name: gradient}) for the loss sum(pooler_output * cotangent)"""
    q = operands(p, bf16, device)
    out = forward(q, input_ids, attention_mask, bf16, pool)
    (out["pooler_output"] * cotangent.to(F64)).sum().backward()
    return {k: v.detach() for k, v in out.items()}, {k: q[k].grad for k in GRAD_KEYS}


# ----------------------------------------------------------------------------------------------------------------------
# kernel-level expectations (exact)
# ----------------------------------------------------------------------------------------------------------------------
def gather_expected(table, ids, rows, D, Dpad, dtype):
    """tan_embed_gather: out [rows, Dpad] = table[ids] (ids outside [0, V) read row 0; ids None = the identity) cast to dtype, the
    pad columns +0"""
    V = table.shape[0]
    if ids is None:
        ids = torch.arange(rows, device=table.device)
    ids = torch.where((ids < 0) | (ids >= V), torch.zeros_like(ids), ids)
    out = torch.zeros(rows, Dpad, dtype=dtype, device=table.device)
    out[:, :D] = table[ids, :D].to(dtype)
    return out


def wordpool_expected(h, mask, dtype):
    """tan_wordpool_fwd on h [M, W, H] of `dtype`: pooled (the selected element; -6e4 as dtype rounds it where every word is masked)
    and argmax int32"""
    pooled, first = first_max(h, mask)
    return pooled.to(dtype), first.to(torch.int32)


def wordpool_bwd_expected(d_pooled, pooled, argmax, W):
    """tan_wordpool_bwd: dh [M, W, H] = d_pooled at (m, argmax[m, j], j) where pooled[m, j] > 0, +0 elsewhere; the gated d_pooled whose
    column sum is the bias gradient, float64"""
    M, H = pooled.shape
    gated = torch.where(pooled.float() > 0, d_pooled, torch.zeros_like(d_pooled))
    dh = torch.zeros(M, W, H, dtype=d_pooled.dtype, device=d_pooled.device)
    dh.scatter_(1, argmax.long()[:, None, :], gated[:, None, :])
    return dh, gated.to(F64)


def rel_err(got, ref):
    got, ref = got.to(F64).reshape(-1), ref.to(F64).reshape(-1)
    den = ref.norm().item()
    return (got - ref).norm().item() / den if den > 0 else got.norm().item()


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def exact_params(p):
    """p with the fc1 path on grids: table entries multiples of 1/8, fc1.weight of 1/64, fc1.bias of 1/512 (fc2 as it is).

    Why: the pooling picks ONE word per (sentence, channel) and the whole gradient of that channel goes through it.  With random
    operands, two words whose h differ by less than the rounding error of an f32 dot product are ordered by that error, and float64
    orders them the other way -- at 2048 x 2048 selections this happens (MI355X, fp32, synth.w2v_params: two selections out of 4 194 304,
    float64 gaps 4.5e-8 and 4.7e-8, which alone put fc1.weight's gradient 3.9e-4 from the reference; with the kernel's own selection
    it is 4.4e-7 away).  That is a property of arg-max, not of a kernel.  On these grids every product is a multiple of 2^-9 with
    at most 9 significant bits and every partial sum of a row stays below 2^24 units (`assert_h_exact`), so h is EXACT in f32 in any
    order of accumulation, the operands are exact in bf16 too, and the stored bf16 h is the rounding of the same exact value in
    the kernel and in the reference: the selection is decided by the first-index rule alone, and exact ties between different words
    are common."""
    q = {k: torch.as_tensor(v).detach().float().clone() for k, v in p.items()}
    q["word_embd.weight"] = (q["word_embd.weight"] * 8).round() / 8
    q["fc1.weight"] = (q["fc1.weight"] * 64).round() / 64
    q["fc1.bias"] = (q["fc1.bias"] * 512).round() / 512
    return q


def assert_h_exact(p):
    """the conditions under which relu(x fc1.weight^T + fc1.bias) is exact in f32 for every row x of the table, from the data"""
    t, w, b = p["word_embd.weight"].double(), p["fc1.weight"].double(), p["fc1.bias"].double()
    for x, unit, nbits in ((t, 8, 4), (w, 64, 5)):
        assert bool((x * unit == (x * unit).round()).all()) and float((x * unit).abs().max()) < 2 ** nbits       # 4 + 5 = 9-bit products
        assert torch.equal(x, x.bfloat16().double())
    assert bool((b * 512 == (b * 512).round()).all())
    assert float(((t.abs() @ w.abs().t()) + b.abs()).max()) * 512 < 2 ** 24            # every partial sum, in units of 2^-9
def tokens(seed, M, W, V):
    """[M, W] int64 ids in [1, V) with ragged lengths >= 1 and trailing zeros, one unknown word (id 0) inside a sentence and, from three
    sentences on, one sentence of zeros only; the attention mask (ids != 0) uint8"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (M, W), generator=g)
    lens = torch.randint(1, W + 1, (M,), generator=g)
    ids[torch.arange(W)[None, :] >= lens[:, None]] = 0
    if M > 2:
        ids[2] = 0
    if W > 3:
        ids[min(1, M - 1), 2] = 0
        ids[min(1, M - 1), 3] = max(1, V // 2)
    return ids, (ids != 0).to(torch.uint8)


def masks(M, W, seed):
    """[M, W] uint8 for the pooling kernel itself, sentence m of kind m % 5: a hole in the middle, a masked first word, every word
    masked (handed to the kernel as it is), every word kept, random"""
    g = torch.Generator().manual_seed(seed)
    k = torch.ones(M, W, dtype=torch.uint8)
    for m in range(M):
        kind = m % 5
        if kind == 0:
            k[m, W // 3:max(W // 3 + 1, 2 * W // 3)] = 0
        elif kind == 1:
            k[m, 0] = 0
        elif kind == 2:
            k[m] = 0
        elif kind == 4:
            k[m] = (torch.rand(W, generator=g) < 0.6).to(torch.uint8)
    return k


def tied_h(M, W, H, dtype, mask, seed):
    """h [M, W, H] of `dtype` full of exact ties: values on a grid of 1/4 (so equal maxima between unmasked words are common), every
    fourth channel clamped at 0 from below, every eighth channel 0 for every word (what the ReLU leaves where no word fires), and in
    channels 1 mod 8 the value -6e4 -- as dtype rounds it -- on the unmasked words of every third sentence: in f32 an exact tie with
    the fill of the masked words before and after it"""
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(M, W, H, generator=g) * 4).round() / 4
    h[:, :, 0::4] = h[:, :, 0::4].clamp(min=0)
    h[:, :, 0::8] = 0
    if mask is not None:
        h[0::3, :, 1::8] = FILL
    return h.to(dtype)
