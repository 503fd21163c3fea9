"""Shape evaluation (recom_amd/csrc/fcp_plan_shape.cc, evaluate_shapes) restated in plain Python, and the requests it is held
to: what a plan makes of a request's offsets, shapes and symbols — the per-column records, the weights' offsets, the arena
layout, the regular-CSR decision and the launch geometry — or the status and message it refuses the request with.

The restatement follows the rule as the library's general routine stated it before the two routines became one: by PLAN
column, rows first, then the layout, records stored at the column's concat position.  The fault texts below were copied
from that routine (compute_dyn_slow, compute_weights).  Test data only."""
import dataclasses
import os

import numpy as np

from recom_amd import lib as _lib
from recom_amd.plan import (COMBINER_MEAN, COMBINER_SQRTN, COMBINER_SUM, FORM_BATCH_COL_REDUCTION, FORM_EXTERNAL, FORM_GATHER,
                            FORM_GATHER_SCATTER, FORM_PASSTHROUGH, FORM_SEGMENT_REDUCE, IDS_I32, IDS_I64, LAYOUT_CONCAT,
                            LAYOUT_PER_COLUMN, ROWS_FROM_GROUP, ROWS_FROM_IDS, ROWS_FROM_INPUT_DIM0, ROWS_FROM_SYMBOL, SEG_CSR_I32,
                            SEG_IDS_I32, SEG_NONE, ColumnSpec, PlanSpec)

WAVE, WAVES_PER_BLOCK = 64, 4
SEG_SEARCH_MAX_PAIRS = 32768          # fcp::Env::seg_search_max_pairs

# ---- the refusals, status and text -------------------------------------------------------------------------------------
SHAPE, ARG, UNSUP = _lib.FCP_ERR_SHAPE_MISMATCH, _lib.FCP_ERR_INVALID_ARGUMENT, _lib.FCP_ERR_UNSUPPORTED
NEG_DIM = (SHAPE, "negative dimension in concated_shapes")
NEG_OFFSET = (SHAPE, "negative blob offset (int32 overflow?)")
PAST_BLOB = lambda i: (SHAPE, f"host input {i} exceeds the blob")
NO_SYMBOLS = (ARG, "plan needs the symbols tensor")
ROWS_RANGE = (SHAPE, "row count out of range")
ROWS_DISAGREE = lambda g: (SHAPE, f"columns of concat group {g} disagree on the row count")
NO_COLUMNS = (ARG, "concat group without columns")
UNALIGNED = (UNSUP, "blob tensor not 4-byte aligned")
PASSTHROUGH_SIZE = (SHAPE, "passthrough tensor size != rows*dim")
PASSTHROUGH_SLOTS = (UNSUP, "passthrough tensor exceeds 2^32 slots")
BCR_SHAPE = (SHAPE, "BatchColReduction shape mismatch")
TOO_MANY_IDS = (UNSUP, "more than 2^31 ids in one column")
GATHER_COUNT = (SHAPE, "gather column: ids count != rows")
CSR_COUNT = (SHAPE, "CSR offsets must have rows+1 entries")
SEG_SHORT = (SHAPE, "segment id tensor shorter than the id stream")
INDEX_SHORT = (SHAPE, "index matrix shorter than the id stream")
MAP_SYMBOL = (SHAPE, "segment-id map: symbol value out of range")
MAP_OVERFLOW = (UNSUP, "segment-id map: factor x symbol exceeds 2^31 (the reshaped row index would overflow)")
CSR_SCRATCH = (UNSUP, "CSR scratch exceeds 2^31 entries")
GRID = (UNSUP, "grid too large")
WEIGHTS_COUNT = lambda k: (SHAPE, f"column {k}: the weights tensor does not hold one weight per id")


class Refused(Exception):
    def __init__(self, answer):
        super().__init__(answer[1])
        self.answer = answer


def align128(x):
    return (x + 127) // 128 * 128


def round32(x):
    return (x + 31) // 32 * 32


# ---- what the plan decides once -----------------------------------------------------------------------------------------
def plan_facts(spec: PlanSpec, max_pairs: int = SEG_SEARCH_MAX_PAIRS) -> dict:
    cols, nc = spec.columns, spec.n_columns
    vec = 4
    for c in cols:
        if c.dim % 4:
            vec = 1 if c.dim % 2 else min(vec, 2)
    order = sorted(range(nc), key=lambda k: (cols[k].concat_group, cols[k].concat_slot))
    pos_of = {k: pos for pos, k in enumerate(order)}
    pooled = lambda c: c.form in (FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER)
    seg_cols = [k for k, c in enumerate(cols) if pooled(c) and c.seg_kind != SEG_CSR_I32]
    seg_cols = [k for k in seg_cols if cols[k].form != FORM_GATHER_SCATTER] + [k for k in seg_cols if cols[k].form == FORM_GATHER_SCATTER]
    has_map = any(len(c.seg_mul) for c in cols)
    has_inverse = any(c.form == FORM_GATHER_SCATTER and c.seg_kind != SEG_CSR_I32 for c in cols)
    seg_search = spec.shard_world <= 1 and not has_map and not has_inverse and \
        not any(c.seg_kind != SEG_NONE and c.seg_stride > 0xffff for c in cols)
    csr_by_pos = spec.layout == LAYOUT_CONCAT and spec.n_groups == 1 and not has_inverse and bool(seg_cols) and \
        2 * len(seg_cols) >= nc and not any(pooled(c) and c.seg_kind == SEG_CSR_I32 for c in cols)
    weighted = any(c.weights_input >= 0 or c.combiner == COMBINER_SQRTN for c in cols)
    width = [spec.group_width(g) for g in range(spec.n_groups)]
    nslots = [w // vec for w in width]
    out_off = spec.column_offsets()
    # hybrid dispatch: every 64-slot span of a group is dense (gathers, passthroughs, external slots only) or ragged; the two
    # lists of all groups lie behind one another in one array
    list_off, list_n, at = [[], []], [[], []], 0
    for g in range(spec.n_groups):
        nspans = (nslots[g] + WAVE - 1) // WAVE
        ragged = [1 if weighted else 0] * nspans
        for k, c in enumerate(cols):
            if c.concat_group == g and c.form not in (FORM_GATHER, FORM_PASSTHROUGH, FORM_EXTERNAL):
                for sp in range(out_off[k] // vec // WAVE, (out_off[k] + c.dim - 1) // vec // WAVE + 1):
                    if sp < nspans:
                        ragged[sp] = 1
        for kind in (0, 1):
            list_off[kind].append(at)
            list_n[kind].append(sum(1 for r in ragged if r == kind))
            at += list_n[kind][-1]
    return dict(vec=vec, order=order, pos_of=pos_of, seg_cols=seg_cols, seg_search=seg_search, csr_by_pos=csr_by_pos, width=width,
                nslots=nslots, out_off=out_off, list_off=list_off, list_n=list_n, max_pairs=max_pairs,
                slot_map_off=[sum(nslots[:g]) for g in range(spec.n_groups)], has_weights=any(c.weights_input >= 0 for c in cols))


# ---- one request ---------------------------------------------------------------------------------------------------------
def evaluate(spec: PlanSpec, facts: dict, offsets, shapes, symbols, blob_bytes: int = -1) -> dict:
    """-> {key: [ints]} with the keys tests/native/plan_shape_san.cc prints; raises Refused((status, message))."""
    cols, nc, ng = spec.columns, spec.n_columns, spec.n_groups
    shape_off = spec.shape_offsets()
    dims = lambda i: [int(v) for v in shapes[shape_off[i]:shape_off[i] + spec.host_input_ranks[i]]]
    numel = []
    for i in range(spec.n_host_inputs):
        if any(d < 0 for d in dims(i)):
            raise Refused(NEG_DIM)
        numel.append(int(np.prod(dims(i), dtype=object)) if dims(i) else 1)
        if offsets[i] < 0:
            raise Refused(NEG_OFFSET)
        if blob_bytes >= 0 and int(offsets[i]) + numel[i] * spec.host_input_elem_sizes[i] > blob_bytes:
            raise Refused(PAST_BLOB(i))

    def own_rows(c):
        if c.rows_source == ROWS_FROM_IDS:
            rows = numel[c.ids_input]
        elif c.rows_source == ROWS_FROM_SYMBOL:
            if symbols is None:
                raise Refused(NO_SYMBOLS)
            rows = int(symbols[c.rows_arg])
        else:
            rows = dims(c.rows_arg)[0]
        if not 0 <= rows <= 0x7fffffff:
            raise Refused(ROWS_RANGE)
        return rows

    # a group's rows: its first column in concat order that is no external slot; the others must agree
    group_rows = []
    for g in range(ng):
        own = [k for k in facts["order"] if cols[k].concat_group == g and cols[k].form != FORM_EXTERNAL]
        if not own:
            raise Refused(NO_COLUMNS)
        group_rows.append(own_rows(cols[own[0]]))
    for k in facts["order"]:
        if cols[k].form != FORM_EXTERNAL and own_rows(cols[k]) != group_rows[cols[k].concat_group]:
            raise Refused(ROWS_DISAGREE(cols[k].concat_group))

    concat = spec.layout == LAYOUT_CONCAT
    out_elem = spec.out_elem_size
    cursor, group_base = 0, [0] * ng
    if concat:
        for g in range(ng):
            group_base[g] = cursor
            cursor += align128(group_rows[g] * facts["width"][g] * out_elem)
    rec, wts = [None] * nc, [-1] * nc
    max_seg_nnz = max_lookup_nnz = seg_pairs = gathered = 0
    for k in (facts["order"] if concat else range(nc)):       # (the per-column layout's cursor runs in plan column order)
        c, rows = cols[k], group_rows[cols[k].concat_group]
        external = c.form == FORM_EXTERNAL
        d = dict(ids_off=0 if external else int(offsets[c.ids_input]), seg_off=0, csr_base=-1, inner=1, rows=rows, seg_sym=1)
        n_ids = 0 if external else numel[c.ids_input]
        if d["ids_off"] % 4:
            raise Refused(UNALIGNED)
        if external:
            d["nnz"] = 0
        elif c.form == FORM_PASSTHROUGH:
            if n_ids != rows * c.dim:
                raise Refused(PASSTHROUGH_SIZE)
            if n_ids // facts["vec"] >= 0xFFFFFFFD:
                raise Refused(PASSTHROUGH_SLOTS)
            d["nnz"] = rows
        elif c.form == FORM_BATCH_COL_REDUCTION:
            s = dims(c.ids_input)
            if s[0] != rows or s[2] != c.dim:
                raise Refused(BCR_SHAPE)
            d["inner"], d["nnz"] = s[1], rows
        else:
            if n_ids > 0x7fffffff:
                raise Refused(TOO_MANY_IDS)
            d["nnz"] = n_ids
            max_lookup_nnz = max(max_lookup_nnz, n_ids)
            if c.form == FORM_GATHER:
                if n_ids != rows:
                    raise Refused(GATHER_COUNT)
            else:
                d["seg_off"] = int(offsets[c.seg_input])
                if d["seg_off"] % 4:
                    raise Refused(UNALIGNED)
                n_seg = numel[c.seg_input]
                if c.seg_kind == SEG_CSR_I32:
                    if n_seg != rows + 1:
                        raise Refused(CSR_COUNT)
                else:
                    if n_ids > 0 and n_seg < n_ids * c.seg_stride - (c.seg_stride - 1):
                        raise Refused(SEG_SHORT)
                    if len(c.seg_mul):
                        if n_seg < n_ids * c.seg_stride:
                            raise Refused(INDEX_SHORT)
                        if c.seg_sym >= 0:
                            if symbols is None:
                                raise Refused(NO_SYMBOLS)
                            d["seg_sym"] = int(symbols[c.seg_sym])
                            if d["seg_sym"] < (1 if c.seg_sym_slot == 4 else 0):
                                raise Refused(MAP_SYMBOL)
                            factor = c.seg_div if c.seg_sym_slot == 4 else c.seg_mul[c.seg_sym_slot]
                            if d["seg_sym"] > 0 and factor > (2 ** 31 - 1) // d["seg_sym"]:
                                raise Refused(MAP_OVERFLOW)
                    max_seg_nnz = max(max_seg_nnz, n_ids)
                    seg_pairs += rows
        if concat:
            d["out_base"] = group_base[c.concat_group] + facts["out_off"][k] * out_elem
            d["out_stride"] = facts["width"][c.concat_group]
        else:
            d["out_base"], d["out_stride"] = cursor, c.dim
            cursor += align128(rows * c.dim * 4)
        gathered += d["nnz"] * c.dim
        if c.weights_input >= 0:
            if numel[c.weights_input] != n_ids:
                raise Refused(WEIGHTS_COUNT(k))
            if offsets[c.weights_input] % 4:
                raise Refused(UNALIGNED)
            wts[facts["pos_of"][k]] = int(offsets[c.weights_input])
        rec[facts["pos_of"][k]] = d
    seg_search = facts["seg_search"] and seg_pairs <= facts["max_pairs"]
    csr_arena_off, csr = cursor, 0
    if facts["csr_by_pos"]:
        stride = round32(group_rows[0] + 1)
        for k in facts["seg_cols"]:
            rec[facts["pos_of"][k]]["csr_base"] = facts["pos_of"][k] * stride
        csr = stride * nc
    else:
        for k in facts["seg_cols"]:
            rec[facts["pos_of"][k]]["csr_base"] = csr
            csr += round32(group_rows[cols[k].concat_group] + 1)
    if csr > 0x7fffffff:
        raise Refused(CSR_SCRATCH)
    # regular CSR: one group with rows; 1 = the scratch by position, filled by the pre-pass; 2 = every column brings CSR
    # offsets and the arrays lie one stride (whole int32s, at least rows + 1 of them) apart in position order
    reg = [0, 0, 0]
    if ng == 1 and nc and group_rows[0] > 0:
        if facts["csr_by_pos"]:
            if not seg_search:
                reg = [1, round32(group_rows[0] + 1), 0]
        elif all(cols[k].seg_kind == SEG_CSR_I32 and cols[k].form in (FORM_SEGMENT_REDUCE, FORM_GATHER_SCATTER) for k in range(nc)):
            seg = [r["seg_off"] for r in rec]
            steps = {b - a for a, b in zip(seg, seg[1:])} or {4 * (group_rows[0] + 1)}
            stride = steps.pop()
            if not steps and stride >= 4 * (group_rows[0] + 1) and stride % 4 == 0 and stride // 4 <= 0x7fffffff and seg[0] % 4 == 0:
                reg = [2, stride // 4, seg[0]]
    out = {f"dyn.{pos}": [r[f] for f in ("ids_off", "seg_off", "out_base", "out_stride", "nnz", "csr_base", "inner", "rows", "seg_sym")]
           for pos, r in enumerate(rec)}
    if facts["has_weights"]:
        out["wts"] = wts
    out.update(group_rows=group_rows, group_base=group_base, arena_bytes=[cursor + 4 * csr], csr_arena_off=[csr_arena_off],
               max_seg_nnz=[max_seg_nnz], max_lookup_nnz=[max_lookup_nnz], seg_pairs=[seg_pairs], seg_search=[int(seg_search)],
               csr_reg=reg, work_bytes=[gathered * 4 + csr_arena_off])
    # launch geometry per kernel kind (0 dense, 1 ragged): the dense kernel takes 1 / 2 / 4 rows per wave below 32 / below 64
    # / from 64 rows of the largest group, the ragged kernel one; a block is 4 waves; a group's listed spans are dealt in
    # eights (nsp8 eights; fewer than 8: -nlist, at least -1) and every span takes one block per row tile
    for kind in (0, 1):
        rpw = 1 if kind == 1 or max(group_rows) < 32 else 2 if max(group_rows) < 64 else 4
        blocks = 0
        for g in range(ng):
            nlist = facts["list_n"][kind][g]
            nspans = (facts["nslots"][g] + WAVE - 1) // WAVE
            nsp8 = (nlist + 7) // 8 if nlist >= 8 else -max(nlist, 1)
            out[f"geo.{kind}.{g}"] = [group_rows[g], facts["nslots"][g], nlist, -1 if nlist == nspans else facts["list_off"][kind][g], nsp8,
                                      blocks, facts["slot_map_off"][g]]
            tiles = (group_rows[g] + WAVES_PER_BLOCK * rpw - 1) // (WAVES_PER_BLOCK * rpw)
            blocks += 0 if nlist == 0 else (8 * nsp8 if nsp8 > 0 else nlist) * tiles
            if blocks > 0x7fffffff:
                raise Refused(GRID)
        out[f"geo.{kind}"] = [rpw, blocks]
    return out


# ---- the requests --------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    spec: PlanSpec
    offsets: np.ndarray
    shapes: np.ndarray
    symbols: "np.ndarray | None"
    blob_bytes: int
    max_pairs: int = -1               # FCP_SEG_SEARCH_MAX_PAIRS at plan creation, -1: unset
    fault: "tuple | None" = None      # the (status, message) this request must be answered with

    def restated(self):
        """{key: [ints]}, or (status, message)"""
        try:
            return evaluate(self.spec, plan_facts(self.spec, SEG_SEARCH_MAX_PAIRS if self.max_pairs < 0 else self.max_pairs),
                            self.offsets, self.shapes, self.symbols, self.blob_bytes)
        except Refused as e:
            return e.answer


def _pack(name, spec, inputs, symbols, **kw) -> Case:
    """The request as Addons>ConcatInputs packs it: the real offsets and concated_bytes."""
    from recom_amd.ops import concat_inputs
    blob, offsets, shapes = concat_inputs(inputs)
    return Case(name, spec, np.array(offsets, np.int32), np.array(shapes, np.int32),
                None if symbols is None else np.array(symbols, np.int32), int(blob.size), **kw)


def _of_model(name, m, seed=0, B=None, **kw) -> Case:
    req = m.make_request(seed) if B is None else m.make_request(seed, B)
    return _pack(name, m.spec, req.inputs, req.symbols, **kw)


def agreement_models():
    """The six synthetic models of the host test of the arena sizes (tests/test_host.py)."""
    from recom_amd import synth
    return [("mixed", synth.model_mixed(batch=21, vocab=97, n_groups=2)), ("s1", synth.model_s1()),
            ("ragged_csr", synth.model_ragged(columns=40, batch=17)), ("ragged_idx", synth.model_ragged(columns=9, batch=5, seg="indices")),
            ("dlrm", synth.model_dlrm(batch=33)), ("ae_e", synth.model_ae("E", batch=19))]


def external_spec(m):
    """model_mixed with an external slot behind group 1 (test_external_slots_host_side)."""
    ext = dataclasses.replace(m.spec.columns[0], form=FORM_EXTERNAL, dim=20, vocab=0, table_input=-1, ids_input=-1, id_source=0,
                              rows_source=ROWS_FROM_GROUP, rows_arg=0, concat_group=1, concat_slot=99)
    return dataclasses.replace(m.spec, columns=m.spec.columns + [ext])


def good_cases():
    import segmap_cases
    import weighted_bag_cases as W
    from recom_amd import synth
    out = []
    for name, m in agreement_models():
        out += [_of_model(f"{name}-seed{seed}", m, seed) for seed in range(3)]
    mixed = synth.model_mixed(batch=21, vocab=97, n_groups=2)
    # the per-column layout with the concat slots reversed: plan column order is not concat order
    top = max(c.concat_slot for c in mixed.spec.columns)
    per_col = dataclasses.replace(mixed.spec, layout=LAYOUT_PER_COLUMN,
                                  columns=[dataclasses.replace(c, concat_slot=top - c.concat_slot) for c in mixed.spec.columns])
    req = mixed.make_request(1)
    out.append(_pack("per_column-permuted", per_col, req.inputs, req.symbols))
    out.append(_pack("external_slot", external_spec(mixed), req.inputs, req.symbols))
    mapped, _, ins_m, _, _, symbols = segmap_cases.build(1)
    out.append(_pack("segmap-symbols", mapped, ins_m, symbols))
    for cell in (W.FormCell(4, "wmean", "idx64"), W.FormCell(1, "wsum", "csr")):
        case = W.form_case(cell)
        out.append(_pack("weighted-" + cell.id, case.spec, *case.requests[1]))
    # one group, every column with CSR offsets: the arrays one stride apart (regular, mode 2), and the last one 8 bytes on
    regular = synth.grouped_csr_model(synth.model_ragged(columns=6, batch=9))
    out.append(_of_model("csr_inputs-regular", regular, 2))
    moved = _of_model("csr_inputs-one_displaced", regular, 2)
    moved.offsets[-1] += 8
    moved.blob_bytes += 8
    out.append(moved)
    ragged = synth.model_ragged(columns=9, batch=5, seg="indices")           # 9 x 5 (column, row) pairs
    out += [_of_model("seg_pairs-at_the_limit", ragged, 0, max_pairs=45), _of_model("seg_pairs-over_the_limit", ragged, 0, max_pairs=44)]
    out += [_of_model(f"mixed-rows{B}", mixed, 3, B) for B in (0, 1, 31, 32, 63, 64)]
    out.append(_of_model("s1-10_spans", synth.model_s1(columns=150, batch=8), 0))    # 600 slots: 10 spans, more than one eight
    return out


def _fault_spec(rows_from_symbol=False, factor=1):
    """One group, one column of every kind a fault can name, and a host input no column reads.
    inputs: 0 ids[B] | 1 payload[B, 3] | 2 payload[B, T, 4] | 3 ids[n] 4 csr[B + 1] | 5 ids[n] 6 seg[n] | 7 ids[n] 8 idx[n, 2] 9 weights[n] |
            10 ids[B] | 11 int8[5], unread;   symbols: 0 the map's factor, 1 B"""
    rows = dict(rows_source=ROWS_FROM_SYMBOL, rows_arg=1) if rows_from_symbol else dict(rows_source=ROWS_FROM_INPUT_DIM0, rows_arg=0)
    look = dict(vocab=50, id_source=IDS_I32)
    cols = [ColumnSpec(FORM_GATHER, 4, table_input=0, ids_input=0, concat_slot=0, rows_source=ROWS_FROM_IDS, **look),
            ColumnSpec(FORM_PASSTHROUGH, 3, ids_input=1, concat_slot=1, **rows),
            ColumnSpec(FORM_BATCH_COL_REDUCTION, 4, ids_input=2, concat_slot=2, **rows),
            ColumnSpec(FORM_SEGMENT_REDUCE, 8, combiner=COMBINER_SUM, table_input=1, ids_input=3, seg_input=4, seg_kind=SEG_CSR_I32,
                       concat_slot=3, **look, **rows),
            ColumnSpec(FORM_SEGMENT_REDUCE, 8, combiner=COMBINER_MEAN, table_input=2, ids_input=5, seg_input=6, seg_kind=SEG_IDS_I32,
                       concat_slot=4, **look, **rows),
            ColumnSpec(FORM_SEGMENT_REDUCE, 4, combiner=COMBINER_SUM, table_input=3, ids_input=7, seg_input=8, seg_kind=SEG_IDS_I32,
                       seg_stride=2, seg_mul=(factor,), seg_sym=0, seg_sym_slot=0, weights_input=9, concat_slot=5, **look, **rows),
            ColumnSpec(FORM_GATHER, 4, table_input=0, ids_input=10, concat_slot=6, **look, **rows)]
    spec = PlanSpec(cols, [1, 2, 3, 1, 1, 1, 1, 1, 2, 1, 1, 1], [4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 1], n_device_inputs=4, n_symbols=2)
    spec.validate()
    return spec


def _fault_inputs(B=6, T=2, n=9):
    i32, f32 = np.int32, np.float32
    seg = np.sort(np.arange(n) % B).astype(i32)
    return [np.arange(B, dtype=i32), np.ones((B, 3), f32), np.ones((B, T, 4), f32), np.arange(n, dtype=i32),
            np.searchsorted(seg, np.arange(B + 1)).astype(i32), np.arange(n, dtype=i32), seg, np.arange(n, dtype=i32),
            np.stack([seg, np.zeros(n, i32)], axis=1), np.ones(n, f32), np.arange(B, dtype=i32), np.zeros(5, np.int8)], np.array([1, B], i32)


def fault_cases():
    """One fault per request (the last case none: an unread input may lie anywhere)."""
    out = []

    def add(name, fault, inputs=None, symbols="kept", spec=None, after=None):
        ins, sym = _fault_inputs()
        for i, a in (inputs or {}).items():
            ins[i] = a
        case = _pack("fault-" + name, spec or _fault_spec(), ins, sym if isinstance(symbols, str) else symbols, fault=fault)
        if after:
            after(case)
        out.append(case)

    def shift(i, by):
        def f(case):
            case.offsets[i] += by
            case.blob_bytes += 8          # (room behind the blob: the shifted input still ends inside it)
        return f

    def set_shape(case):
        case.shapes[case.spec.shape_offsets()[2] + 1] = -1
    i32, f32 = np.int32, np.float32
    ins, _ = _fault_inputs()
    add("negative_dimension", NEG_DIM, after=set_shape)
    add("negative_offset", NEG_OFFSET, after=lambda case: case.offsets.__setitem__(3, -4))
    add("past_the_blob", PAST_BLOB(11), after=lambda case: setattr(case, "blob_bytes", int(case.offsets[11]) + 5 - 1))
    add("ids_unaligned", UNALIGNED, after=shift(10, 2))
    add("segments_unaligned", UNALIGNED, after=shift(6, 2))
    add("weights_unaligned", UNALIGNED, after=shift(9, 2))
    add("rows_disagree", ROWS_DISAGREE(0), {10: np.arange(7, dtype=i32)}, spec=dataclasses.replace(
        _fault_spec(), columns=_fault_spec().columns[:6] + [dataclasses.replace(_fault_spec().columns[6], rows_source=ROWS_FROM_IDS)]))
    by_symbol = _fault_spec(True)          # (its map without the symbol: the rows' symbol is the only one the plan needs)
    add("no_symbols-rows", NO_SYMBOLS, symbols=None, spec=dataclasses.replace(
        by_symbol, columns=by_symbol.columns[:5] + [dataclasses.replace(by_symbol.columns[5], seg_sym=-1)] + by_symbol.columns[6:]))
    add("no_symbols-map", NO_SYMBOLS, symbols=None)
    add("gather_count", GATHER_COUNT, {10: np.arange(7, dtype=i32)})
    add("passthrough_size", PASSTHROUGH_SIZE, {1: np.ones((6, 4), f32)})
    add("bcr_shape", BCR_SHAPE, {2: np.ones((6, 2, 5), f32)})
    add("csr_count", CSR_COUNT, {4: np.append(ins[4], ins[4][-1]).astype(i32)})
    add("segments_short", SEG_SHORT, {6: ins[6][:-1]})
    add("index_matrix_short", INDEX_SHORT, {8: np.zeros((2 * 9 - 1, 1), i32)})
    add("map_symbol_range", MAP_SYMBOL, symbols=np.array([-1, 6], i32))
    add("map_overflow", MAP_OVERFLOW, symbols=np.array([2 ** 30, 6], i32), spec=_fault_spec(factor=4))
    add("weights_count", WEIGHTS_COUNT(5), {9: np.ones(10, f32)})
    add("rows_range", ROWS_RANGE, symbols=np.array([1, -1], i32), spec=_fault_spec(True))
    add("unread_input_at_an_odd_offset", None, after=shift(11, 1))
    return out


def all_cases():
    return good_cases() + fault_cases()


def write_requests(path: str, cases, plan_dir: str) -> None:
    """The requests as text for tests/native/plan_shape_san.cc, each with its plan as a column-plan file in `plan_dir`."""
    from recom_amd import plan_io
    ints = lambda a: f"{len(a)} " + " ".join(str(int(v)) for v in a)
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for i, c in enumerate(cases):
            plan = os.path.join(plan_dir, f"shape_case_{i}.plan")
            plan_io.save_plan(c.spec, plan)
            f.write(f"{c.name} {plan} {c.max_pairs} {c.blob_bytes} {ints(c.offsets)} {ints(c.shapes)} "
                    f"{'-1' if c.symbols is None else ints(c.symbols)}\n")


def parse_output(text: str) -> dict:
    """What plan_shape_san printed -> {case: {key: [ints]} or (status, message)}"""
    out, name = {}, None
    for line in text.splitlines():
        key, _, rest = line.partition(" ")
        if key == "case":
            name = rest
            out[name] = {}
        elif key == "status":
            if int(rest):
                out[name] = (int(rest), None)
        elif key == "message":
            out[name] = (out[name][0], rest)
        elif key != "end":
            out[name][key] = [int(v) for v in rest.split()]
    return out
