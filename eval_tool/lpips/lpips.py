"""The reference's eval_tool/lpips/lpips.py surface: ``LPIPS(net_type='alex', version='0.1')`` on the HIP kernels (reface_amd/lpips.py).

Differences from the reference, all about where the weights come from: the constructor downloads nothing -- every parameter is zero until
``load_state_dict`` (the reference module's keys and shapes) or the optional keyword ``ckpt=`` (reface_amd.lpips.load_lpips_state: a state
dict file, a REFace checkpoint with ``lpips_loss.*`` keys, or "none" for the seeded weights of the tests).  'squeeze' is not implemented.
``forward`` takes fp32 NCHW device tensors in [-1, 1]; host tensors raise, as every op here rejects them.

The engines pack the weights once.  ``forward`` notices when the module's tensors have changed since (an in-place write, ``.to(...)``,
``load_state_dict``: every parameter's storage, dtype and version counter are compared) and packs them again."""
import torch
import torch.nn as nn

from eval_tool.lpips.networks import LinLayers, get_network

VERSIONS = ("0.1",)


class LPIPS(nn.Module):
    def __init__(self, net_type="alex", version="0.1", ckpt=None):
        super().__init__()
        assert version in VERSIONS, "v0.1 is only supported now"
        self.net_type = net_type
        self.net = get_network(net_type)
        self.lin = LinLayers(self.net.n_channels_list)
        self._scorer, self._packed = None, None
        if ckpt is not None:
            from reface_amd.lpips import load_lpips_state
            self.load_state_dict(load_lpips_state(ckpt, net_type))

    def _fingerprint(self, device):
        return (str(device),) + tuple((k, v.data_ptr(), v._version, v.dtype) for k, v in self.state_dict(keep_vars=True).items())

    def forward(self, x, y):
        from reface_amd.lpips import LPIPSScorer
        if not (torch.is_tensor(x) and torch.is_tensor(y) and x.is_cuda and y.is_cuda):
            from reface_amd._lib import RefaceHipError
            raise RefaceHipError("reface_amd ops need device tensors (no CPU fallback)")
        now = self._fingerprint(x.device)
        if self._scorer is None or self._packed != now:
            self._scorer, self._packed = LPIPSScorer(self.state_dict(), net=self.net_type, device=x.device), now
        totals = self._scorer.distances(x, y).totals
        return (totals[0] / totals[1]).to(torch.float32)          # the sum over pairs and layers over the batch size
