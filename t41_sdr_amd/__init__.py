"""t41_sdr_amd -- MI355X-native T41 receive DSP hot path (ProcessIQData) behind a C ABI.

Only what the path needs lives here: csrc/ (HIP kernels + C++ host side + C ABI) and rx.py (the
host-side mirror of the reference interface).  Importing the package does not need a GPU;
creating an RxChain does.
"""
from ._lib import (DEMOD_AM, DEMOD_LSB, DEMOD_NFM, DEMOD_SAM, DEMOD_USB, LIB_PATH, Params, T41RxError,  # noqa: F401
                   load)
from ._lib import SETS_STAGES, STAGE_ALL, STAGE_CW_DECODE, STAGE_CW_DETECT, STAGE_EQ, STAGE_NB, STAGE_NR  # noqa: F401
from .rx import RxChain, blob_fields, blob_params, default_params, design_coeffs, ft8_tables, param_sets_compatible  # noqa: F401
from . import beacon  # noqa: F401
from . import ft8  # noqa: F401
from . import panadapter  # noqa: F401
from .tx import TxChain, TxParams, cal_tone, default_tx_params, sine_tone  # noqa: F401

__all__ = ["RxChain", "Params", "T41RxError", "default_params", "design_coeffs", "blob_fields", "load",
           "DEMOD_USB", "DEMOD_LSB", "DEMOD_AM", "DEMOD_NFM", "DEMOD_SAM", "LIB_PATH"]
