from .resources import load_audio, load_audio_wavPCM, resample  # noqa: F401
