"""flash_attn.flash_attn_interface: the variable-length packed-QKV entry point with upstream's signature."""
from gaussiancity_amd.attention import varlen_qkvpacked


def flash_attn_varlen_qkvpacked_func(qkv, cu_seqlens, max_seqlen, dropout_p=0.0, softmax_scale=None, causal=False,
                                     window_size=(-1, -1), softcap=0.0, alibi_slopes=None, deterministic=False,
                                     return_attn_probs=False):
    """qkv [total, 3, heads, head_dim] float16, cu_seqlens int32 [segments + 1] -> [total, heads, head_dim] float16.
    Plain softmax attention inside every segment; the variants below are refused by name.  `deterministic` is
    accepted and ignored: the backward pass has no atomics and is always bit-reproducible."""
    if dropout_p > 0:
        raise NotImplementedError("dropout_p > 0 is not supported (got %r)" % (dropout_p,))
    if causal:
        raise NotImplementedError("causal=True is not supported")
    if tuple(window_size) != (-1, -1):
        raise NotImplementedError("window_size other than (-1, -1) is not supported (got %r)" % (window_size,))
    if softcap != 0:
        raise NotImplementedError("softcap != 0 is not supported (got %r)" % (softcap,))
    if alibi_slopes is not None:
        raise NotImplementedError("alibi_slopes is not supported")
    if return_attn_probs:
        raise NotImplementedError("return_attn_probs=True is not supported")
    return varlen_qkvpacked(qkv, cu_seqlens, max_seqlen, softmax_scale)
