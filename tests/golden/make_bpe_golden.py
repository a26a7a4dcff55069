"""Writes tests/golden/clip_bpe_merges.txt.gz: the header line and the first 48 894 merges of
OpenAI CLIP's public bpe_simple_vocab_16e6.txt.gz, which are all that CLIP's 49 408-id vocabulary
uses (lcclip.tokenizer.N_MERGES). The full file is 1.3 MB; this part is 0.2 MB.

  python tests/golden/make_bpe_golden.py <path to bpe_simple_vocab_16e6.txt.gz>
"""
import gzip
import os
import sys

N_MERGES = 49152 - 256 - 2
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "clip_bpe_merges.txt.gz")

with gzip.open(sys.argv[1], "rt", encoding="utf-8") as f:
    lines = f.read().split("\n")
with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, compresslevel=9) as g:
    g.write(("\n".join(lines[:1 + N_MERGES]) + "\n").encode("utf-8"))
print(OUT, os.path.getsize(OUT), "bytes")
