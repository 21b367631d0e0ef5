"""GPU tests (-m gpu) of the compressed-size calls: lzf_compressed_size_batch, lzf_compressed_size_batch_host,
lzf_frame_compressed_size_device, lzf_frame_compress_stream_size_device and the `exact=True` outputs built on them.  The cases are
tests/compressed_size_cases.py's (every expectation pinned to the oracle, every class proven reached by
tests/test_compressed_size_cases_cpu.py); the checks are tests/compressed_size_check.py's, one child process per group.  Exact
integers and statuses throughout; each group reports how many cases it compared, and that number is asserted here."""
import os
import re
import subprocess
import sys
import time

import pytest

import compressed_size_check as chk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", list(chk.GROUPS))
def test_compressed_size_group(group):
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "compressed_size_check.py"), group], capture_output=True, text=True,
                       timeout=300)
    print(f"{group}: {time.time() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-4000:]
    m = re.search(r"^%s ok: (\d+) cases$" % group, r.stdout, re.M)
    assert m and int(m.group(1)) == chk.COUNTS[group], r.stdout[-2000:]
