"""MI355X-native (gfx950) forward/backward path for the Daft-Exprt acoustic model.

Public surface mirrors the reference (src/daft_exprt/model.py, loss.py): ``DaftExprt``, ``DaftExprtLoss``,
``HyperParams``.  The compute is in ``libdaft_exprt_hip.so`` (hand-written HIP, C ABI in include/daft_exprt_hip.h);
importing the model classes does not need a GPU, running them does.
"""
from .hparams import HyperParams  # noqa: F401
from .model import DaftExprt  # noqa: F401
from .loss import DaftExprtLoss  # noqa: F401
from .functional import manual_seed  # noqa: F401
from .ops import set_precision, get_precision, Runtime  # noqa: F401
from .vocoder import HiFiGANGenerator, HiFiGanVocoder, VocoderStream, load_hifigan_vocoder, stream_plan  # noqa: F401
from .vocoder import v1_config, v2_config, v3_config, workspace_bytes_per_frame  # noqa: F401
from .vocoder_train import backward_launches  # noqa: F401
from .mel import MelSpectrogram, mel_filter_bank, mel_spectrogram, mel_spectrogram_HiFi  # noqa: F401
from .griffin_lim import GriffinLim, GriffinLimVocoder, griffin_lim_reconstruction_from_mel_spec  # noqa: F401
from .speech import SpeechSynthesizer, condition_external_prosody, symbol_prosody, to_pcm16  # noqa: F401
from .discriminators import (DiscriminatorP, DiscriminatorS, HiFiGanDiscriminators, MultiPeriodDiscriminator,  # noqa: F401
                             MultiScaleDiscriminator, discriminator_loss, feature_loss, generator_loss)
from .vocoder_optim import NormedAdamW  # noqa: F401
from .vocoder_finetune import HiFiGanFineTuner  # noqa: F401
from .vocoder_data import HiFiGanFineTuneData  # noqa: F401
