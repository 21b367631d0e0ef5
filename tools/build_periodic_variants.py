"""Analysis builds for the study of the fed kernel's overlapping matches of period 1, 2, 4 and 8 (profiles/fed_periodic_matches.txt)
-> rust-lz-fear_amd/liblzfear_hip_<hash>.so; prints one 'name path' line per build.
  old         -DLZF_FED_NO_PERIODIC: the byte loop with its two divisions for every offset (the kernel before)
  bound       -DLZF_FED_NO_PERIODIC -DLZF_DBG_SKIP=64: the same, and the moves of near overlapping matches of offset 1, 2, 4, 8 left out
              altogether (wrong output by design; lengths and statuses unchanged): against `old`, all that those moves cost
  rounds      -DLZF_DBG_FED_COUNT=3: trips of the match-round loop per job in results[].reserved
  masked      -DLZF_DBG_FED_COUNT=4: overlapping cooperative matches moved without a division, per job (build.FED_PERIODIC_COUNTER_BUILD)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rust_lz_fear_amd  # noqa
from rust_lz_fear_amd import build
VARIANTS = {"old": ["LZF_ANALYSIS", "LZF_FED_NO_PERIODIC"], "bound": ["LZF_FED_NO_PERIODIC", "LZF_DBG_SKIP=64"],
            "rounds": ["LZF_DBG_FED_COUNT=3"], "masked": list(build.FED_PERIODIC_COUNTER_BUILD)}
for name in sys.argv[1:] or list(VARIANTS):
    print(name, build.build_library(defines=VARIANTS[name]), flush=True)
