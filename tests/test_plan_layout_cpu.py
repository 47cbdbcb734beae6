"""The operand layout of a plan record (ctl_op) by name: the "plan record layout" table of include/ctl_hip.h, mirrored by _ffi.OP_LAYOUT
for readers (_ffi.op_field) and hand-built records (_ffi.new_op); the emitters of nets.PlanBuilder still write positions by hand.  Checked
here without a GPU: the two tables agree, the names are parameter names of the entry a record is handed to, the table fits the record, and
the PACK_BATCH and BN_REPLAY records and tables the networks build sit at the positions and in the word order the header states."""
import os
import re

import numpy as np
import pytest

from cooperative_training_and_latent_space_data_augmentation_amd import _ffi, nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ctl_hip.h")).read()
# fields that are not parameters of the entry their line names (the header's table says what they are instead)
NOT_PARAMETERS = {"group_splits", "members", "form"}
INT_WORDS, CONV_WORDS = _ffi.OP_DTYPE["i"].shape[0], _ffi.CONV_DTYPE.itemsize // 4


def header_layout():
    """{kind name: (entry or None, has conv, [(bank, index, name, index was written out)])} from the header's layout lines"""
    out = {}
    for name, entry, banks in re.findall(r"^ \*   ([A-Z0-9_]+)(?: -> (ctl_[a-z0-9_]+))? \|(.*)$", HEADER, flags=re.M):
        fields, conv = [], False
        for bank in banks.split("|"):
            letter, names = bank.split(":")
            k = 0
            for tok in names.split():
                if tok == "conv":
                    conv = True
                elif "=" in tok:
                    fields.append((letter.strip(), int(tok.split("=")[0]), tok.split("=")[1], True))
                else:
                    fields.append((letter.strip(), k, tok, False))
                    k += 1
        assert name not in out, f"{name} has two layout lines"
        out[name] = (entry or None, conv, fields)
    return out


def header_kinds():
    body = re.search(r"enum ctl_op_kind \{(.*?)\};", HEADER, flags=re.S).group(1)
    return {name: int(v) for name, v in re.findall(r"CTL_OP_([A-Z0-9_]+) = (\d+)", body)}


def prototypes():
    """{entry: [parameter names]} with the prototype regex of tests/test_cabi.py"""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S))
    protos = re.findall(r"([A-Za-z_][\w \t\*]*?)\b(ctl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)
    return {name: [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",") if a.strip() not in ("", "void")] for _, name, args in protos}


def test_layout_table_matches_the_header():
    kinds, lines = header_kinds(), header_layout()
    assert len(kinds) == 20 and set(lines) == set(kinds), set(lines) ^ set(kinds)          # a kind without a line fails
    assert set(_ffi.OP_LAYOUT) == set(kinds.values())
    for name, value in kinds.items():
        entry, conv, fields = lines[name]
        lay = _ffi.OP_LAYOUT[value]
        assert getattr(_ffi, "OP_" + name) == value
        assert (lay.name, lay.entry, lay.conv) == (name, entry, conv)
        assert list(lay.fields.items()) == [(n, (bank, k)) for bank, k, n, _ in fields], name          # names, indices and order


def test_field_names_are_parameter_names_of_the_entry():
    """Membership only: every field of a line is SOME parameter of the entry the line names.  That a field sits at the position the
    interpreter hands to THAT parameter is not checked here (two names swapped within a bank pass); the parity suites on the GPU do that."""
    protos = prototypes()
    for name, (entry, conv, fields) in header_layout().items():
        if entry is None:
            assert name in ("WGRAD_GROUP", "ZERO", "COPY")
            continue
        params = protos[entry]
        assert not conv or params[0] in ("d",), (name, entry)          # the ctl_conv of a conv-family record is the entry's descriptor
        for _, _, field, _ in fields:
            assert field in params or field in NOT_PARAMETERS, f"{name}: {field} is no parameter of {entry}{tuple(params)}"
        assert not [f for _, _, f, _ in fields if f in NOT_PARAMETERS and f in params]


def test_layout_table_fits_the_record():
    sizes = {"i": INT_WORDS, "l": _ffi.OP_DTYPE["l"].shape[0], "f": _ffi.OP_DTYPE["f"].shape[0], "t": _ffi.OP_MAX_T}
    assert sizes == {"i": 27, "l": 4, "f": 4, "t": 14} and CONV_WORDS == 24
    for name, (_, conv, fields) in header_layout().items():
        places = [(bank, k) for bank, k, _, _ in fields]
        assert len(set(places)) == len(places), f"{name}: two fields share a position"
        for bank, k, field, written_out in fields:
            assert 0 <= k < sizes[bank], (name, field)
            if bank == "i":
                assert k < CONV_WORDS or written_out, f"{name}: {field} reaches i[{k}] without saying so"
                assert not (conv and k < CONV_WORDS), f"{name}: {field} lies inside the ctl_conv"


@pytest.fixture(scope="module")
def model():
    return nets.build_networks(reduce_factor=4, device="cpu", dtype="fp32")


def test_new_op_writes_named_fields_and_refuses_unknown_names():
    with pytest.raises(KeyError, match="no_such_field"):
        _ffi.new_op(_ffi.OP_BN_ACT, c=16, no_such_field=1)
    with pytest.raises(KeyError):
        _ffi.new_op(_ffi.OP_BN_ACT, _ffi.conv_desc(n=1, hin=8, win=8, cin=16, hout=8, wout=8, cout=16, ks=3), c=16)      # no ctl_conv in a BN_ACT record
    # every field of every kind: written, read back; an omitted tensor reads back as NULL
    for kind, lay in _ffi.OP_LAYOUT.items():
        values = {}
        for n, (field, (bank, k)) in enumerate(lay.fields.items()):
            values[field] = {"t": (1 + n % 5, 256 * (n + 1)), "f": 0.25 * (n + 1)}.get(bank, 1000 + n)
        omitted = [f for f, (bank, _) in lay.fields.items() if bank == "t"][1::2]
        for f in omitted:
            values[f] = None
        d = _ffi.conv_desc(n=2, hin=8, win=8, cin=16, hout=8, wout=8, cout=32, ks=3, dt=_ffi.DT_X3) if lay.conv else None
        rec = _ffi.new_op(kind, d, **values)
        assert int(rec["kind"]) == kind
        for f, v in values.items():
            assert _ffi.op_field(rec, f) == ((-1, 0) if v is None else v), (lay.name, f)
        if lay.conv:
            assert _ffi.op_field(rec, "conv").tobytes() == d.tobytes()
        with pytest.raises(KeyError):
            _ffi.op_field(rec, "no_such_field")
        bare = _ffi.new_op(kind)
        assert all(_ffi.op_field(bare, f) == (-1, 0) for f, (bank, _) in lay.fields.items() if bank == "t")


def raw_record(kind, i=(), l=(), f=(), slots=()):
    r = np.zeros((), dtype=_ffi.OP_DTYPE)
    r["kind"] = kind
    r["slot"][:] = -1
    for k, v in enumerate(i):
        r["i"][k] = v
    for k, v in enumerate(l):
        r["l"][k] = v
    for k, v in enumerate(f):
        r["f"][k] = v
    for k, s in enumerate(slots):
        r["slot"][k] = s
    return r


def header_words(label):
    """the column names of one of the int64 tables, in the word order the header documents ("<label> record (n words): ...;")"""
    m = re.search(label + r" record\s+\((\d+) words\):", HEADER)
    text = re.sub(r"\([^()]*\)", "", HEADER[m.end():m.end() + 1000].replace("\n *", " "))      # the list ends at the first ';' outside parentheses
    names = [w.strip() for w in text.split(";")[0].split(",")]
    assert len(names) == int(m.group(1)) == len(set(names)), (label, names)
    return names


def test_pack_record_sits_at_its_raw_positions(model):
    """the PACK_BATCH record the network builds and two rows of its table, pinned to the positions ctl_plan_run and the pack kernels read;
    the same record rebuilt by name is the same bytes, the same rows listed in the header's word order are the same rows"""
    enc = model["image_encoder"]
    pack = enc._pack_plan
    table = pack.table_np
    assert pack.n_ops == 1 and table.dtype == np.int64 and table.shape[1] == 12
    assert enc._x3_packs                                                       # (the fp32 network at reduce factor 4 has X3 layers)
    want = raw_record(16, i=[len(table), 2], l=[int(table[:, 10].max())], slots=[nets.S_P, nets.S_WP, nets.S_TAB])
    assert pack.ops[0].tobytes() == want.tobytes()
    cols = header_words("pack")
    named = _ffi.new_op(_ffi.OP_PACK_BATCH, n_rec=len(table), form=2, max_total=int(table[:, cols.index("total")].max()),
                        params=(nets.S_P, 0), wpack=(nets.S_WP, 0), table=(nets.S_TAB, 0))
    assert named.tobytes() == want.tobytes()
    ci = next(iter(enc._convs.values()))                                       # the first conv's forward pack is the first row
    assert not ci.transposed
    k2 = ci.ks * ci.ks
    total = _ffi.lib.ctl_conv_wpack_floats(ci.cin, ci.cout, ci.ks)
    assert table[0].tolist() == [ci.w_off, ci.wp_fwd, ci.cout, ci.cin, ci.ks, 0, ci.cin * k2, k2, ci.ks, 1, total, 0]
    by_name = dict(src_off=ci.w_off, dst_off=ci.wp_fwd, cout=ci.cout, cin=ci.cin, ks=ci.ks, flip=0, s_co=ci.cin * k2, s_ci=k2, s_kh=ci.ks, s_kw=1,
                   total=total, mode=0)
    assert table[0].tolist() == [by_name[c] for c in cols]
    c4 = [r for r in table if r[11] == 4]                                      # the K-packed first-layer row
    assert len(c4) == 1 and c4[0].tolist() == [ci.w_off, ci.wp_c4, ci.cout, ci.cin, 3, 0, ci.cin * k2, k2, ci.ks, 1, ((ci.cout + 15) // 16) * 3 * 256, 4]


def test_replay_record_sits_at_its_raw_positions(model):
    """the BN_REPLAY record and table CtlNet.replay_running_stats builds, pinned the same way.  The plan is built before it is run, and on
    device="cpu" the run is refused before anything is launched: what is left in Plan.replay is the record under test."""
    import types
    dec = model["segmentation_decoder"]
    fwd = dec._compile_forward(2, 3, 4, "A")
    assert fwd.replay is None and len(fwd.bn_log) > 0
    with pytest.raises(_ffi.CtlError, match="needs the network on a GPU"):
        dec.replay_running_stats((types.SimpleNamespace(t=None), fwd))
    replay = fwd.replay
    assert replay.n_ops == 1
    want = raw_record(19, i=[len(fwd.bn_log)], f=[nets.MOMENTUM], slots=[nets.S_ACT, nets.S_B, nets.S_NBT, nets.S_TAB])
    assert replay.ops[0].tobytes() == want.tobytes()
    named = _ffi.new_op(_ffi.OP_BN_REPLAY, n_rec=len(fwd.bn_log), momentum=nets.MOMENTUM, act=(nets.S_ACT, 0), buffers=(nets.S_B, 0),
                        num_batches_tracked=(nets.S_NBT, 0), table=(nets.S_TAB, 0))
    assert named.tobytes() == want.tobytes()
    rows = np.array([[co["mean"][1], co["uvar"][1], bn.rm_off, bn.rv_off, bn.nbt_idx, bn.c] for bn, co in fwd.bn_log], dtype=np.int64)
    assert replay.table_np.dtype == np.int64 and np.array_equal(replay.table_np, rows)
    cols = header_words("replay")
    by_name = [dict(save_mean_off=co["mean"][1], save_uvar_off=co["uvar"][1], running_mean_off=bn.rm_off, running_var_off=bn.rv_off,
                    nbt_idx=bn.nbt_idx, c=bn.c) for bn, co in fwd.bn_log]
    assert replay.table_np.tolist() == [[r[c] for c in cols] for r in by_name]


def test_reduce_row_names_follow_the_header_and_a_real_table(model):
    assert list(_ffi.ReduceRow._fields) == header_words("reduce")
    dec = model["segmentation_decoder"]
    bwd = dec._compile_backward(dec._compile_forward(2, 3, 4, "A"), "A", (True,), True, True, True)
    rows = {r.w_off: r for r in map(_ffi.ReduceRow._make, bwd.table_np.tolist())}
    own = [o for o in bwd.ops if int(o["kind"]) == _ffi.OP_WGRAD and _ffi.op_field(o, "group_splits") == 0]
    assert own and len(rows) == len(bwd.table_np)
    for o in own:                                                              # a launch of its own: the library's split count
        d = _ffi.op_field(o, "conv")
        r = rows[_ffi.op_field(o, "w_partial")[1] // 4]
        cin, cout, ks = int(d["cin"]), int(d["cout"]), int(d["ks"])
        assert (r.cin, r.cout, r.taps_ks, r.cin_p, r.cout_p) == (cin, cout, ks * ks | ks << 8, -(-cin // 16) * 16, -(-cout // 16) * 16)
        assert r.splits == _ffi.lib.ctl_wgrad_splits(_ffi.desc_ptr(np.atleast_1d(d))) and r.reserved == 0 and r.accumulate in (0, 1)
        assert (r.b_off >= 0) == (_ffi.op_field(o, "b_partial")[0] >= 0) == (r.db_off >= 0) and r.dw_off >= 0
