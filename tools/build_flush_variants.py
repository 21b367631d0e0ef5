"""Builds for the study of the fed kernel's deferred flush (profiles/fed_deferred_flush.txt) -> rust-lz-fear_amd/liblzfear_hip_<hash>.so;
prints one 'name path' line per build.
  noflush     -DLZF_DBG_SKIP=16: no flush and no drain (wrong output by design; lengths and statuses unchanged)
  dry         -DLZF_DBG_SKIP=128: the deferred flush's ring reads and address work without its stores (wrong output by design)
  fences      -DLZF_DBG_FED_COUNT=5: store fences in front of a batch's far / slow sources, per job in results[].reserved"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_lz_fear_amd  # noqa
from rust_lz_fear_amd import build
VARIANTS = {"noflush": ["LZF_DBG_SKIP=16"], "dry": ["LZF_DBG_SKIP=128"], "fences": ["LZF_DBG_FED_COUNT=5"]}
for name in sys.argv[1:] or list(VARIANTS):
    print(name, build.build_library(defines=VARIANTS[name]), flush=True)
