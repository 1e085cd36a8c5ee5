"""ddsp.training, as far as it is built: `nn` (the note pooling, the layers of RnnFcDecoder and the normalisations), `decoders`
(RnnFcDecoder), `encoders` (the z encoders) and `preprocessing` (the scalings and F0LoudnessPreprocessor)."""
from ddsp_amd.training import nn
from ddsp_amd.training import decoders
from ddsp_amd.training import encoders
from ddsp_amd.training import preprocessing
