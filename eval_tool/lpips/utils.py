"""The reference's eval_tool/lpips/utils.py surface: ``normalize_activation`` and ``get_state_dict``.

``normalize_activation`` is the plain formula, kept as a public helper; the engine's normalisation runs inside rf_lpips_layer
(reface_amd/csrc/lpips.hip).  ``get_state_dict`` downloads the linear weights in the reference; nothing here touches the network."""
import torch


def normalize_activation(x, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True) + 1e-16)
    return x / (norm_factor + eps)


def get_state_dict(net_type: str = 'alex', version: str = '0.1'):
    raise RuntimeError(f"eval_tool.lpips.utils.get_state_dict('{net_type}', '{version}'): the published LPIPS weights are not downloaded here. "
                       "Load them from a file instead: LPIPS(net_type, ckpt=PATH), module.load_state_dict(...), or --lpips_ckpt PATH of "
                       "eval_tool/lpips/lpips_compare.py (a state dict of the LPIPS module, or a REFace checkpoint holding lpips_loss.* keys)")
