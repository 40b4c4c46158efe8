"""The names of the reference's eval_tool/lpips/networks.py -- ``get_network``, ``LinLayers``, ``AlexNet``, ``VGG16`` -- as parameter holders.

The modules carry the reference's state-dict keys and shapes (``mean``, ``std``, ``layers.<i>.{weight,bias}``; ``<l>.1.weight``), zero until
a state dict is loaded; nothing is downloaded.  They do not compute: the feature stacks run on the HIP kernels through
``eval_tool.lpips.lpips.LPIPS.forward`` (reface_amd/lpips.py).  Which nets exist, their layers and the errors for the others come from
``reface_amd.params.lpips_plan``."""
import torch
import torch.nn as nn

from reface_amd.params import LPIPS_CHANNELS, lpips_plan

TARGET_LAYERS = {"alex": [2, 5, 8, 10, 12], "vgg": [4, 9, 16, 23, 30]}          # 1-based module positions of the taps, as the reference lists them


class _Holder(nn.Module):
    """Frozen parameters of one convolution."""

    def __init__(self, weight_shape, bias_shape=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(weight_shape), requires_grad=False)
        if bias_shape is not None:
            self.bias = nn.Parameter(torch.zeros(bias_shape), requires_grad=False)


class LinLayers(nn.ModuleList):
    """One bias-free 1x1 convolution per tap, at index 1 of its entry (the reference's entries are Sequential(Identity, Conv2d))."""

    def __init__(self, n_channels_list):
        super().__init__(nn.ModuleDict({"1": _Holder((1, int(c), 1, 1))}) for c in n_channels_list)


class BaseNet(nn.Module):
    """The buffers and convolution parameters of one backbone, keyed as torchvision's ``features`` keys them."""

    def __init__(self, net_type):
        plan = lpips_plan(net_type)          # raises NotImplementedError for 'squeeze' and for unknown names
        super().__init__()
        self.net_type = net_type
        self.register_buffer("mean", torch.zeros(1, 3, 1, 1))
        self.register_buffer("std", torch.zeros(1, 3, 1, 1))
        self.layers = nn.ModuleDict({str(i): _Holder((cout, cin, k, k), (cout,)) for kind, i, cin, cout, k, _, _ in (p for p in plan if p[0] == "conv")})
        self.target_layers = list(TARGET_LAYERS[net_type])
        self.n_channels_list = list(LPIPS_CHANNELS[net_type])

    def forward(self, x):
        raise NotImplementedError("the feature stack runs inside eval_tool.lpips.lpips.LPIPS.forward (HIP kernels); this module holds its parameters")


class AlexNet(BaseNet):
    def __init__(self):
        super().__init__("alex")


class VGG16(BaseNet):
    def __init__(self):
        super().__init__("vgg")


_NETS = {"alex": AlexNet, "vgg": VGG16}


def get_network(net_type):
    """The parameter holder of 'alex' or 'vgg'."""
    if net_type not in _NETS:
        lpips_plan(net_type)          # the error for 'squeeze' / an unknown name
    return _NETS[net_type]()
