"""`from sim_src.alg.gm import MAX_GAIN, MAX_ASSO, MAX_RAND` -> the device greedy baselines (sig_sdp_mmw_amd.gm)."""
from sig_sdp_mmw_amd.gm import MAX_ASSO, MAX_GAIN, MAX_RAND  # noqa: F401
