"""Source-level contracts of the library's host code (no GPU, no build needed):

* every environment switch of smirk_amd/csrc is read through smirk_switch (capi.hip), the only getenv of the library, and is listed in the table of
  switches.h and named in INTEGRATION.md;
* the dynamic-LDS opt-in (hipFuncSetAttribute) is made in one place, smirk_raise_dynamic_lds (capi.hip);
* no -DSMIRK_DEBUG_HOOKS instrumentation is left in the library or its tools.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "smirk_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc():
    return {f: _read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def _calls(name):
    return [(f, m.start()) for f, s in _csrc().items() for m in re.finditer(r"\b%s\s*\(" % name, s)]


def _switch_names():
    enum = re.search(r"enum SmirkSwitch \{(.*?)\};", _read(os.path.join(CSRC, "switches.h")), re.S).group(1)
    return ["SMIRK_" + n for n in re.findall(r"SMIRK_SW_(\w+)", enum) if n != "COUNT"]


def test_getenv_only_in_smirk_switch():
    calls = _calls("getenv")
    assert len(calls) == 1 and calls[0][0] == "capi.hip", calls
    capi = _read(os.path.join(CSRC, "capi.hip"))
    body = capi[capi.index("int smirk_switch(SmirkSwitch s)"):]
    assert body.index("getenv(") < body.index("\n}\n")


def test_switch_table():
    names = _switch_names()
    assert len(names) == 11 and len(set(names)) == 11
    capi = _read(os.path.join(CSRC, "capi.hip"))
    listed = re.findall(r'"(SMIRK_\w+)"', re.search(r"names\[\] = \{(.*?)\};", capi, re.S).group(1))
    assert listed == names                                     # smirk_switch's name list follows the enum
    table = _read(os.path.join(CSRC, "switches.h")).split("#pragma once")[0]
    integration = _read(os.path.join(REPO, "INTEGRATION.md"))
    for n in names:
        assert re.search(r"^// %s\s" % n, table, re.M), n
        assert re.search(r"`%s`" % n, integration), n


def test_dynamic_lds_opt_in_in_one_place():
    calls = _calls("hipFuncSetAttribute")
    assert len(calls) == 1 and calls[0][0] == "capi.hip", calls
    capi = _read(os.path.join(CSRC, "capi.hip"))
    body = capi[capi.index("int smirk_raise_dynamic_lds("):]
    assert body.index("hipFuncSetAttribute(") < body.index("\n}\n")


def test_no_debug_hooks():
    hits = []
    for top in ("smirk_amd", "tools"):
        for root, _, files in os.walk(os.path.join(REPO, top)):
            for f in files:
                if f.endswith((".hip", ".h", ".py", ".sh", ".md")) and "SMIRK_DEBUG_HOOKS" in _read(os.path.join(root, f)):
                    hits.append(os.path.join(root, f))
    assert not hits, hits
