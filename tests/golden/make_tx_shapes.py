#!/usr/bin/env python3
"""Generate tests/golden/tx_shapes.json from the REFERENCE's own transmitter
(oracle/_ref/minimodem_ref, built by `make -C oracle` where the reference's sources exist):

    python tests/golden/make_tx_shapes.py

One record per `minimodem --tx --file` command line of tests/_txshapes.py: the arguments, how
many samples the reference wrote and the SHA-256 of them as float32 (an S16 file read back as
libsndfile reads it).  Left out, and counted on stdout: configurations that mifsk_rx_config_init
refuses (the receive side's limits: no transmitter test can build them), and command lines on
which the reference itself aborts (a tone of no samples trips its assert).  Nothing of the
product's output goes into the file.  tests/test_tx_shapes.py replays it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import _oracle as O  # noqa: E402
import _txshapes as T  # noqa: E402
import minimodem_amd as M  # noqa: E402


def record(line, payload, wav):
    """The reference on one command line -> a record, or None where it aborts."""
    r = subprocess.run([O.MINIMODEM_REF, "--tx", "--file", wav] + line.split(), input=payload,
                       stderr=subprocess.DEVNULL)
    if r.returncode != 0:
        return None
    _sr, x = O.read_wav(wav)
    return {"args": line, "n": int(x.shape[0]), "sha256": T.digest(x)}


def main():
    assert O.have_ref(), "needs oracle/_ref (make -C oracle where the reference's sources are)"
    fd, wav = tempfile.mkstemp(suffix=".wav", prefix="txshapes-")
    os.close(fd)
    records, refused, aborted = [], 0, 0
    try:
        for line in T.sweep_lines():
            cfg_kw, _ = T.parse(line)
            try:
                M.rx_config(**cfg_kw)
            except ValueError:
                refused += 1
                continue
            rec = record(line, T.PAYLOAD, wav)
            if rec is None:
                aborted += 1
                continue
            records.append(rec)
        baudot = []
        for line in T.BAUDOT_LINES:
            rec = record(line, T.BAUDOT_TEXT, wav)
            assert rec is not None, line
            baudot.append(rec)
    finally:
        os.unlink(wav)
    with open(T.FIXTURE, "w") as f:
        f.write('{"payload": "%s",\n "baudot_text": %s,\n "records": [\n' %
                (T.PAYLOAD.hex(), json.dumps(T.BAUDOT_TEXT.decode("ascii"))))
        f.write(",\n".join("  " + json.dumps(r) for r in records))
        f.write('\n ],\n "baudot_records": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in baudot))
        f.write("\n ]}\n")
    print("%d records + %d baudot, %d refused by rx_config, %d aborted in the reference; %s %d bytes" %
          (len(records), len(baudot), refused, aborted, T.FIXTURE, os.path.getsize(T.FIXTURE)))


if __name__ == "__main__":
    main()
