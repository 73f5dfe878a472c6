"""scripts/isa_loop.py's listing rule (one round trip per trip): from a main-loop trip's
first record load on, the child-ref load (buffer_load_dwordx2 ... offset:48) is issued before any
s_waitcnt that can hold the wave for this trip's records.  No GPU and no compiler: the rule runs over
small listings in the assembler's own form -- the shape the depth-1 kernels have, the earlier shape
(a masked load in a region of its own above the inner-step branch), and three broken ones -- and the
script's exit status follows it."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "isa_loop.py")

HEAD = """\
.LBB1_4:                                ; =>This Inner Loop Header: Depth=1
	v_cmp_gt_i32_e64 s[2:3], 0, v42
	s_waitcnt vmcnt(2)
	v_lshlrev_b32_e32 v2, 6, v42
	buffer_load_dwordx4 v[2:5], v43, s[44:47], 0 offen
	buffer_load_dwordx4 v[10:13], v43, s[44:47], 0 offen offset:16
	buffer_load_dwordx4 v[6:9], v43, s[44:47], 0 offen offset:32
	ds_read_b32 v52, v53
"""
TAIL = """\
	v_pk_add_f32 v[2:3], v[2:3], v[26:27] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]
	s_waitcnt vmcnt(0)
	v_add_u32_e32 v15, v54, v15
	s_cbranch_execnz .LBB1_4
"""
REF = "\tbuffer_load_dwordx2 v[42:43], v43, s[44:47], 0 offen offset:48\n"
INNER = "; %bb.5:                                ;   in Loop: Header=BB1_4 Depth=1\n"

LISTINGS = {
    # the ref load first in the inner step's region; the first wait allows the three loads before it
    "lean": (HEAD + "\ts_and_saveexec_b64 s[0:1], vcc\n" + INNER + REF + "\ts_waitcnt vmcnt(3)\n" + TAIL, True),
    # the earlier form: a wait that holds nobody (vmcnt(3) after three loads), then the masked ref load
    "early": (HEAD + "\ts_waitcnt vmcnt(3)\n\tv_mov_b32_e32 v47, 0\n\ts_and_saveexec_b64 s[0:1], vcc\n" + INNER + REF +
              "\ts_or_b64 exec, exec, s[0:1]\n\ts_waitcnt vmcnt(2)\n" + TAIL, True),
    # the ref load behind the inner step's first wait
    "behind the wait": (HEAD + "\ts_and_saveexec_b64 s[0:1], vcc\n" + INNER + "\ts_waitcnt vmcnt(2)\n" + REF + TAIL, False),
    # behind a wait for everything
    "behind vmcnt(0)": (HEAD + "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n" + REF + TAIL, False),
    # no ref load at all
    "missing": (HEAD + TAIL, False),
}


def _module():
    spec = importlib.util.spec_from_file_location("isa_loop", SCRIPT)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_ref_load_rule_on_listings():
    m = _module()
    for name, (text, holds) in LISTINGS.items():
        got, line = m.ref_load_rule(text.splitlines())
        assert got == holds, (name, line)
        assert ("holds" in line) == holds and ("BROKEN" in line) != holds, (name, line)
    # a wait on the LDS counter alone, or one before the trip's first load, is no wait on the records
    ok = HEAD.replace("\tds_read_b32 v52, v53\n", "\tds_read_b32 v52, v53\n\ts_waitcnt lgkmcnt(0)\n") + REF + TAIL
    assert m.ref_load_rule(ok.splitlines())[0]


def test_the_scripts_exit_status_follows_the_rule(tmp_path):
    """The script end to end on a one-kernel file: status 0 and 'holds' in the census, status 1 and
    'BROKEN' when the ref load sits behind the wait."""
    for name in ("lean", "behind the wait"):
        text, holds = LISTINGS[name]
        asm = tmp_path / "k.s"
        asm.write_text("_Z6kernelv: ; @_Z6kernelv\n; %bb.0:\n\ts_mov_b64 s[50:51], 0\n" + text +
                       "; %bb.9:\n\ts_endpgm\n.Lfunc_end0:\n")
        out = tmp_path / "census"
        res = subprocess.run([sys.executable, SCRIPT, str(asm), "_Z6kernelv", str(out)], capture_output=True, text=True, timeout=60)
        assert (res.returncode == 0) == holds, (name, res.returncode, res.stderr[-500:])
        census = open(str(out) + ".txt").read()
        assert ("ref load rule: holds" in census) == holds and ("ref load rule: BROKEN" in census) != holds, census
