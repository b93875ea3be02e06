"""whisperx_amd — MI355X-native forced alignment + VAD segmentation for WhisperX.

Drop-in for the reference's alignment path (whisperx/__init__.py:2 re-exports
load_align_model/align) and its VAD post-processing (whisperx/vad.py Binarize,
merge_chunks).  Compute runs in libwxalign.so (HIP, gfx950); see DESIGN.md.
"""
import os as _os

# wav2vec2's convolutions see a new input length for almost every VAD chunk.  MIOpen's
# default find mode searches (and JIT-compiles) kernels per new shape: ~1.2 s each on a
# fresh MI355X; FAST picks by heuristic (~10 ms forward for a 30 s chunk either way).
# Set before the first convolution; a user's own setting wins.
_os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
from .alignment import (  # noqa: F401
    DEFAULT_ALIGN_MODELS_HF,
    DEFAULT_ALIGN_MODELS_TORCH,
    LANGUAGES_WITHOUT_SPACES,
    PUNKT_ABBREVIATIONS,
    Point,
    Segment,
    align,
    backtrack,
    get_trellis,
    load_align_model,
    merge_repeats,
    merge_words,
)
from .audio import (  # noqa: F401
    CHUNK_LENGTH,
    FRAMES_PER_SECOND,
    HOP_LENGTH,
    N_FFT,
    N_FRAMES,
    N_SAMPLES,
    N_SAMPLES_PER_TOKEN,
    SAMPLE_RATE,
    TOKENS_PER_SECOND,
    load_audio,
    log_mel_chunks,
    log_mel_spectrogram,
    mel_filters,
    pad_or_trim,
)
from .vad import Binarize, merge_chunks  # noqa: F401
from .diarize import assign_word_speakers, assign_word_speakers_batch  # noqa: F401
from .writers import get_writer, format_timestamp  # noqa: F401
from .whisper import DecodingResult, Hypothesis, WhisperDecoder, WhisperEncoder, load_whisper_decoder, load_whisper_encoder  # noqa: F401
from .integration import install  # noqa: F401

__version__ = "0.1.0"
