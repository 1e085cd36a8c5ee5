"""ddsp.training, as far as it is built: the pure tensor functions of `nn` that pool features over notes."""
from ddsp_amd.training import nn
