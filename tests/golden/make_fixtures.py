"""Regenerates the reference-derived fixtures.  Runs ONLY in the build container, where the
reference tree is mounted at /root/reference; nothing here travels except the outputs.

  python tests/golden/make_fixtures.py
"""
import collections
import glob
import gzip
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_ffi as o  # noqa: E402

REF = "/root/reference"
FUZZ_CORPORA = ("decode", "interop_decode", "roundtrip_fuzz")
# Two frames of the decode corpus carry text, Cargo.toml.lz4 (a package manifest) and README.md.lz4 (a code sample among
# the prose), and many of its other files are mutations of them.  A file is left out of the packed corpus when its bytes, or
# what it decodes to, share a run of TEXT_WINDOW printable characters with the decoded text of either frame.
TEXT_FRAMES = ("Cargo.toml.lz4", "README.md.lz4")
TEXT_WINDOW = 4


def printable_windows(b):
    out = set()
    for run in re.findall(rb"[\x20-\x7e\t\n]{%d,}" % TEXT_WINDOW, b):
        out.update(run[i:i + TEXT_WINDOW] for i in range(len(run) - TEXT_WINDOW + 1))
    return out


def carries_text(data, text_windows):
    rc, dec, _ = o.frame_decompress(data)
    return bool((printable_windows(data) | printable_windows(dec or b"")) & text_windows)


def main():
    # 1. issue-15 data vector (tests/issue-15.rs:5)
    src = open(os.path.join(REF, "tests", "issue-15.rs")).read()
    m = re.search(r"let input = \[(.*?)\];", src, re.S)
    vals = bytes(int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{2})", m.group(1)))
    assert len(vals) == 81248
    open(os.path.join(HERE, "issue15_input.bin"), "wb").write(vals)

    # 2. the one corpus frame that is pure data (random bytes, stored block)
    shutil.copyfile(os.path.join(REF, "fuzz/corpus/decode/uncomp.data.lz4"), os.path.join(HERE, "uncomp.data.lz4"))

    # 3. fingerprints of the valid frames + census of the whole decode corpus
    out = {"valid_frames": {}, "census": {}}
    census = collections.Counter()
    per_file = {}
    for f in sorted(glob.glob(os.path.join(REF, "fuzz/corpus/decode/*"))):
        data = open(f, "rb").read()
        rc, dec, used = o.frame_decompress(data)
        name = o.STATUS_NAMES[rc]
        census[name] += 1
        per_file[os.path.basename(f)] = name
        if rc == 0 and os.path.basename(f).endswith(".lz4"):
            out["valid_frames"][os.path.basename(f)] = {
                "in_len": len(data), "in_xxh32": "%08x" % o.xxh32(data),
                "out_len": len(dec), "out_xxh32": "%08x" % o.xxh32(dec)}
    out["census"] = dict(sorted(census.items()))
    out["per_file"] = per_file
    json.dump(out, open(os.path.join(HERE, "corpus_frames.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out["census"], indent=1), out["valid_frames"])

    # 4. the fuzz corpora themselves (data: the inputs of the fuzz targets), packed: one gzip-ed concatenation per corpus
    #    directory, files in name order, and an index of (name, length); tests/test_oracle.py unpacks them (fuzz_corpus()).
    #    The decode corpus without the files that carry text (TEXT_FRAMES above): their names are listed as left out.
    text_windows = set()
    for n in TEXT_FRAMES:
        rc, dec, _ = o.frame_decompress(open(os.path.join(REF, "fuzz/corpus/decode", n), "rb").read())
        assert rc == 0
        text_windows |= printable_windows(dec)
    index = {}
    for d in FUZZ_CORPORA:
        files = sorted(glob.glob(os.path.join(REF, "fuzz/corpus", d, "*")))
        text = [f for f in files if carries_text(open(f, "rb").read(), text_windows)]
        if d == "decode":
            index["decode_left_out"] = [os.path.basename(f) for f in text]
            files = [f for f in files if f not in text]
        else:
            assert not text, (d, text)                  # the plaintext corpora carry none of it
        index[d] = [[os.path.basename(f), os.path.getsize(f)] for f in files]
        with open(os.path.join(HERE, f"fuzz_{d}.bin.gz"), "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as gz:
                for f in files:
                    gz.write(open(f, "rb").read())
    json.dump(index, open(os.path.join(HERE, "fuzz_corpus.json"), "w"), indent=0)
    print({d: len(v) for d, v in index.items()})


if __name__ == "__main__":
    main()
