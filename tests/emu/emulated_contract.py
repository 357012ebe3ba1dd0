#!/usr/bin/env python3
"""The device-pointer contract (tests/device_contract.py) against the emulated kernels built with AddressSanitizer / UBSan:
every registry row whose device code the library holds, every buffer malloc'ed at EXACTLY its size ("tight" arenas), so that
a load or store of the device code one word outside a caller's buffer is an AddressSanitizer report and a 16-byte access at
a 4-byte-aligned address a UBSan one.  AFX_LIB = the library tests/test_device_contract_emulated.py builds.
Arguments: row names ("entry[ident]") or nothing for all; "--list" prints them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import device_contract as dc  # noqa: E402


def main(argv):
    todo = [r for r in dc.rows(emulated=True, env=bool(os.environ.get("AFX_CONTRACT_ENV_ROWS")))
            if not argv or str(r) in argv or r.entry in argv]
    if argv == ["--list"]:
        print("\n".join(str(r) for r in dc.rows(emulated=True)))
        return
    for r in todo:
        for k, v in (r.env or {}).items():
            os.environ[k] = v
        dc.check_row(r, "tight", quick=True)
        for k in (r.env or {}):
            os.environ.pop(k, None)
        print(f"contract {r}: extent, poisoned surroundings, alignment, history, value anchor", flush=True)
    print(f"rows: {len(todo)}\nOK")


if __name__ == "__main__":
    main(sys.argv[1:])
