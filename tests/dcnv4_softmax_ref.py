"""Reference for the DCNv4 operator with ``MDCONV_FLAG_SOFTMAX`` (include/mdconv.h, "DCNv4 operator"): unpack the row in
fp64, take the softmax of the K masks of every (output pixel, group) -- over ALL K tensor taps, whatever the gate does to
them --, repack, and call ``tests.dcnv4_ref.dcnv4_ref``.  Gradients come from autograd, so a gated-out tap's logit takes the
gradient the normaliser gives it.  The padding columns are never looked at (``unpack`` drops them, ``pack`` writes zeros)."""
import torch

from tests import dcnv4_ref as R


def softmax_pack(offset_mask, group, K):
    """The packed tensor with the masks' softmax per (pixel, group) in the place of the logits, fp64; differentiable."""
    B, Ho, Wo, _ = offset_mask.shape
    offset, logits = R.unpack(offset_mask.double(), group, K)
    mask = torch.softmax(logits.reshape(B, Ho, Wo, group, K), -1).reshape(B, Ho, Wo, group * K)
    return R.pack(offset, mask, group, K)


def dcnv4_softmax_ref(input, offset_mask, kernel, stride, pad, dilation, group, group_channels, offset_scale,
                      remove_center=False, softmax=True):
    """fp64 restatement; differentiable.  Returns the result in the dtype of ``input``.  (``softmax`` is accepted so that the
    function can stand in for ``dcnv4_core`` inside the modules; it must be true.)"""
    assert softmax
    om = softmax_pack(offset_mask, group, R.taps(kernel, remove_center))
    return R.dcnv4_ref(input.double(), om, kernel, stride, pad, dilation, group, group_channels, offset_scale,
                       remove_center).to(input.dtype)


def dcnv4_softmax_ref_grads(input, offset_mask, grad_output, *geo):
    """(output, grad_input, grad_offset_mask) in fp64 from the values the tensors hold.  NaN padding columns take no part:
    their gradient is zero."""
    x, om = (t.detach().double().cpu().requires_grad_(True) for t in (input, offset_mask))
    out = dcnv4_softmax_ref(x, om, *geo)
    gi, gom = torch.autograd.grad(out, (x, om), grad_output.detach().double().cpu())
    return out.detach(), gi, gom


def shift_logits(offset_mask, group, K, shift):
    """``offset_mask`` with ``shift`` (a number, or a tensor [B, Ho, Wo, G, 1]) added to the logits of every group, in the
    tensor's dtype."""
    B, Ho, Wo, _ = offset_mask.shape
    offset, logits = R.unpack(offset_mask, group, K)
    logits = (logits.reshape(B, Ho, Wo, group, K).double() + shift).reshape(B, Ho, Wo, group * K).to(offset_mask.dtype)
    out = offset_mask.clone()
    out[..., :group * K * 3] = R.pack(offset, logits, group, K)[..., :group * K * 3]
    return out
