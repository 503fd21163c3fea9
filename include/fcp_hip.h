/*
 * fcp_hip.h — C ABI of libfcp_hip.so: the MI355X-native fused feature-column
 * (embedding-column) inference path.
 *
 * This is the drop-in boundary for the three custom ops of the reference
 * (AlibabaResearch/recom, paths relative to the reference root):
 *
 *   Addons>ConcatInputs                      custom_ops/concat_inputs/concat_inputs_ops.cc:42-88
 *   Addons>FeatureColumnProcess[WithSymbols] custom_ops/feature_column_process/feature_column_process_op_gpu.cu.cc:65-175
 *   Addons>ConcatOutputs[NoHost]             custom_ops/concat_outputs/concat_outputs_op_gpu.cu.cc:180-288
 *
 * and for the `extern "C"` entry points those ops dlsym from the JIT-compiled
 * artifact today:
 *
 *   CreateConstBuffers      graph_optimizers/cuda_emitter.cc:2260-2301
 *   ProcessFeatureColumns   graph_optimizers/cuda_emitter.cc:2303-2494 (decl feature_column_process_ops.h:37-43)
 *   ConcatOutputs           custom_ops/concat_outputs/concat_outputs_op_gpu.cu.cc:133-140 (decl concat_outputs_ops.h:34)
 *
 * The reference entry points are C-named but C++-typed (std::vector,
 * std::function, references).  Here everything is plain C: pointers, sizes,
 * int status codes, function-pointer allocators.  No torch / TF / HIP types
 * appear in any signature (a HIP stream is passed as an opaque pointer).
 *
 * What the reference generates as CUDA text per model (one `struct FCi` per
 * feature column, cuda_emitter.cc:1976-2055) is described here by a static
 * *column plan* (fcp_column_desc_t[]) that pre-compiled gfx950 kernels
 * interpret.  No code generation and no runtime compiler are involved.
 *
 * Threading: a plan is immutable after creation; fcp_process_feature_columns
 * and fcp_concat_outputs are re-entrant on a shared plan (the reference ops
 * keep no per-call state in members either, SURVEY.md §8b "Threading").
 * Concurrent calls (serve workers, one stream each) serialise only on the
 * plan's descriptor-slot bookkeeping; shape evaluation, the allocator callback
 * and the kernel launches of different callers overlap.  No entry point
 * synchronises the stream in the steady state: work is enqueued and the call
 * returns (the reference blocks three times per request).  A
 * call may wait for an EARLIER request's kernel when more than 8 requests with
 * new shapes are in flight (back-pressure on the descriptor slots).
 */
#ifndef FCP_HIP_H_
#define FCP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCP_ABI_VERSION 2 /* 2: id transforms (fcp_column_desc_t::xform_*), external slots, placement gate; additions since keep every v2 struct as it was */

/* ---- status codes (reference: void returns + CubDebugExit/exit(1)) ------ */
enum {
  FCP_OK = 0,
  FCP_ERR_INVALID_ARGUMENT = 1, /* bad descriptor / null pointer / bad enum  */
  FCP_ERR_SHAPE_MISMATCH = 2,   /* run-time shapes inconsistent with the plan */
  FCP_ERR_ALLOC = 3,            /* an allocator callback returned NULL        */
  FCP_ERR_HIP = 4,              /* a HIP runtime call failed                  */
  FCP_ERR_UNSUPPORTED = 5,      /* valid but not implemented for this plan    */
  FCP_ERR_NO_DEVICE = 6         /* no gfx950 device / code object not loadable*/
};

/* ---- column forms: the canonical per-column rewrites of the reference ---- */
/* (lookup_optimizer.cc:157-440; emitter dispatch cuda_emitter.cc:1096-1152)  */
enum {
  /* GatherV2(table, ids): out[i,:] = W[ids[i],:]
   * cuda_emitter.cc:250-293 (GatherRowsToGlbMem), driver :1246-1330 */
  FCP_FORM_GATHER = 1,
  /* SparseSegment{Sum,Mean,SqrtN}[WithNumSegments](table, ids, seg_ids, B)
   * cuda_emitter.cc:402-501, :564-661 (dim<=20) and :768-962 (dim>20); SqrtN and per-id weights
   * (fcp_column_ext_t::weights_input1) have no reference counterpart */
  FCP_FORM_SEGMENT_REDUCE = 2,
  /* ScatterNd(rows, GatherV2(table, ids), [B,dim]): zero-fill, then
   * out[rows[i],:] = W[ids[i],:]   cuda_emitter.cc:296-345, :1332-1442
   * The row ids (seg_kind FCP_SEG_IDS_*) arrive in ANY order, as the reference's
   * kernel takes them; of several writes to one row the LAST one stays (the order
   * of a sequential scatter; the reference races inside a 64-id tile), rows
   * outside [0, B) are dropped (TF's ScatterNd on a GPU) and, with
   * FCP_FLAG_COUNT_BAD_IDS, counted.  The segment-offset pre-pass builds the
   * row -> position map for such columns.  With seg_kind FCP_SEG_CSR_I32 the ids
   * are grouped by row and the last id of a row's range wins.  An id filter
   * (xform) drops ids before the scatter: the last id it KEEPS wins. */
  FCP_FORM_GATHER_SCATTER = 3,
  /* A tensor of the ConcatInputs blob copied straight into its concat slot
   * (ConcatOutputs `host_inputs`, concat_outputs_op_gpu.cu.cc:186-216) */
  FCP_FORM_PASSTHROUGH = 4,
  /* Sum(x, axis=1) on a rank-3 [B,R,C] tensor of the blob
   * cuda_emitter.cc:1180-1244 (BatchColReduction) */
  FCP_FORM_BATCH_COL_REDUCTION = 5,
  /* A concat slot somebody else fills: an Addons>ConcatOutputs `host_inputs`
   * tensor (concat_outputs_op_gpu.cu.cc:186-216; Rewrite wires every non-FC
   * input of the ConcatV2 that way, cuda_emitter.cc:2594-2611).  The plan only
   * reserves [rows, dim] at the slot's concat offset — the kernels never touch
   * it — and fcp_concat_outputs_host copies the host tensor there.  It is NOT an
   * output of FeatureColumnProcess (fcp_plan_output_columns skips it), has no
   * inputs (ids_input = table_input = -1) and takes its row count from its
   * group (FCP_ROWS_FROM_GROUP).  FCP_LAYOUT_CONCAT only. */
  FCP_FORM_EXTERNAL = 6
};

/* The combiners of TensorFlow's embedding columns (embedding_lookup_sparse): the bag's rows are added in id order from
 * +0.0f; MEAN divides by the number of ids that reached the lookup, SQRTN (SparseSegmentSqrtN) by the correctly rounded
 * float32 square root of that number — one IEEE float32 division per element.  With per-id weights
 * (fcp_column_ext_t::weights_input1) the denominators are the sum of the weights and the square root of the sum of
 * their squares.  A zero denominator gives a row of +0.0 (TF's div_no_nan).  SQRTN: FCP_FORM_SEGMENT_REDUCE only. */
enum { FCP_COMBINER_NONE = 0, FCP_COMBINER_SUM = 1, FCP_COMBINER_MEAN = 2, FCP_COMBINER_SQRTN = 3 };

/* How the id stream of a column is stored in the blob (what EmitInputInline
 * folds into the index expression, cuda_emitter.cc:1769-1949). */
enum {
  FCP_IDS_I32 = 0,           /* int32 ids                                    */
  FCP_IDS_I64 = 1,           /* int64 ids (reference truncates to int, :270) */
  FCP_IDS_F32_BUCKETIZE = 2  /* float32 values -> Bucketize(boundaries), :233-247, :1798-1835 */
};

/* Id transform, applied to every id after it has been decoded (raw integer or
 * Bucketize result) and before the lookup: what the CPU ops the
 * reference's PreLookupOptimizer puts in front of the lookup compute
 * (graph_optimizers/pre_lookup_optimizer.cc:596-654).  The interval set is a list of
 * CLOSED integer intervals [lo_i, hi_i] — the ops' left_boundaries / right_boundaries
 * attrs.  An id is "in" when lo_i <= id && id <= hi_i for some i.  (The reference's
 * kernels test `x >= l || x <= r`, select_value_ops.cc:35-41 — true for every x, so
 * they filter nothing; this is the intended test, SURVEY.md App. A.) */
enum {
  FCP_XFORM_NONE = 0,
  /* Addons>SelectValue (custom_ops/select_value/select_value_ops.cc:33-56):
   * id' = in ? id : substitute */
  FCP_XFORM_SELECT = 1,
  /* Addons>GatherIndiceValue / Addons>GatherValueGenIndice
   * (gather_indice_value_ops.cc:33-78, gather_value_gen_indice_ops.cc:33-67): ids that
   * are not "in" are DROPPED: they add nothing to their row and do not count in a
   * mean; a row left without ids is zeros.  (Row-sharded plans: fcp_shard_finalize
   * re-reads the row's ids and divides a mean by the kept count.) */
  FCP_XFORM_FILTER = 2
};

/* How segment membership of the id stream is given. */
enum {
  FCP_SEG_NONE = 0,     /* forms 1,4,5                                        */
  FCP_SEG_IDS_I32 = 1,  /* sorted segment / row ids, element stride seg_stride */
  FCP_SEG_IDS_I64 = 2,  /* e.g. SparseTensor indices[nnz,2] int64 with stride 2
                           (inlined StridedSlice [:,0], cuda_emitter.cc:1836-1873) */
  FCP_SEG_CSR_I32 = 3   /* CSR offsets int32[B+1] (what ComputeSegmentOffsets,
                           cuda_emitter.cc:768-818, produces on the fly)      */
};

/* Where the number of output rows ("prefix size") of a column comes from. */
enum {
  FCP_ROWS_FROM_IDS = 0,    /* rows = number of elements of the ids tensor (form 1) */
  FCP_ROWS_FROM_SYMBOL = 1, /* rows = symbols[rows_arg] (Addons>ShapeConstruct
                               result, cuda_emitter.cc:2438-2455)             */
  FCP_ROWS_FROM_INPUT_DIM0 = 2, /* rows = shape[0] of host input rows_arg      */
  FCP_ROWS_FROM_GROUP = 3   /* FCP_FORM_EXTERNAL: rows of the other columns of its concat group */
};

/* Output arena layouts. */
enum {
  /* One [rows, sum(dim)] row-major matrix per concat group; every column is
   * written directly at its concat offset: ConcatOutputsKnl
   * (concat_outputs_op_gpu.cu.cc:85-131) is fused away. */
  FCP_LAYOUT_CONCAT = 0,
  /* The reference arena: one contiguous [rows, dim] buffer per column, each
   * 128-byte aligned (alignmem, cuda_emitter.cc:967-969, :2151-2179);
   * fcp_concat_outputs then performs the reference's second pass. */
  FCP_LAYOUT_PER_COLUMN = 1
};

enum {
  FCP_FLAG_NONE = 0,
  /* Count ids outside [0, vocab) into the plan's device error counter.  Such
   * rows always read as zeros (TF-GPU GatherV2 semantics); the reference
   * reads out of bounds. */
  FCP_FLAG_COUNT_BAD_IDS = 1u << 0,
  /* Narrow output (FCP_LAYOUT_CONCAT, unsharded): the concat groups are written as bf16 / fp16 instead of float32.
   * A narrow element is fl16(x) of the float32 value x the same plan without the bit would have written, rounded ONCE,
   * to nearest-even, at the store: overflow goes to +-inf (fp16: |x| >= 65520; bf16: the last half-ulp below 2^128),
   * underflow is gradual (subnormals, then zero: float32 subnormals stay bf16 subnormals and become +-0 in fp16),
   * -0.0 stays -0.0, NaN stays NaN (sign and payload unspecified).  The geometry is unchanged IN ELEMENTS — widths,
   * column offsets, output_shapes, group_shapes, output_row_strides — and halves in BYTES: a group occupies
   * rows x width x 2 bytes (128-byte aligned, as ever), output_ptrs / group_ptrs address 2-byte elements, buffer_bytes and
   * fcp_plan_arena_bytes follow, the CSR scratch sits (4-byte aligned) behind the narrow outputs.  At most one of the
   * two bits (both: FCP_ERR_INVALID_ARGUMENT); neither: the float32 plan, bit for bit.  Refused with
   * FCP_ERR_UNSUPPORTED: shard_world > 1 (partial sums cross the exchange in float32), FCP_LAYOUT_PER_COLUMN (the
   * reference's float32 arena), any FCP_FORM_EXTERNAL column (fcp_concat_outputs_host scatters float32 payloads), any
   * column with per-id weights or FCP_COMBINER_SQRTN. */
  FCP_FLAG_OUT_BF16 = 1u << 1,
  FCP_FLAG_OUT_F16 = 1u << 2,
  /* 16-bit tables: EVERY embedding table of the plan (every device input a GATHER / SEGMENT_REDUCE / GATHER_SCATTER
   * column reads) is bf16 / fp16, row-major [vocab, dim], 2 bytes per element, its base 2 * V-byte aligned (V = 4 | 2 | 1:
   * the largest of them dividing every column's dim and offset; 8 bytes always suffice).  A 16-bit element widens to
   * float32 EXACTLY, so the plan computes, bit for bit, what the same plan without the bit computes on the widened tables:
   * gathers, scatters, pooled sums and means in id order from +0.0, range checks, the zeros of ids outside the vocabulary.
   * bf16 widens in integers (pattern << 16: a copied NaN keeps sign and payload); an fp16 NaN widens to some NaN.
   * Everything else is unchanged — the geometry, the float32 output, the blob (PASSTHROUGH / BATCH_COL_REDUCTION payloads
   * stay float32), both layouts, every id source and transform, FCP_FLAG_COUNT_BAD_IDS, 2^32 - 3 rows per table;
   * fcp_plan_table_bytes counts 2 bytes per element.  At most one of the two bits (both: FCP_ERR_INVALID_ARGUMENT);
   * neither: the float32-table plan and its code paths, exactly.  Refused with FCP_ERR_UNSUPPORTED: together with
   * FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16, shard_world > 1, any column with per-id weights or FCP_COMBINER_SQRTN. */
  FCP_FLAG_TABLES_BF16 = 1u << 3,
  FCP_FLAG_TABLES_F16 = 1u << 4,
  /* 8-bit row-quantised tables (the "fused 8-bit rowwise" format of FBGEMM / TorchRec, the tensor PyTorch's
   * quantized::embedding_bag_byte_prepack returns): EVERY embedding table of the plan (every device input a GATHER /
   * SEGMENT_REDUCE / GATHER_SCATTER column reads) is row-major uint8 [vocab, dim + 8], its base 4-byte aligned, no padding
   * between rows: row r starts at byte r * (dim + 8); bytes [0, dim) are the codes, [dim, dim + 4) the float32 scale,
   * [dim + 4, dim + 8) the float32 bias, both little-endian and read correctly at ANY byte alignment (a dim that is no
   * multiple of 4 misaligns them in most rows).  An element dequantises to the float32 value fma(float(code), scale, bias):
   * the product exact, the sum rounded ONCE to nearest-even (what quantized::embedding_bag_byte_unpack computes; NaN and
   * infinity follow IEEE); the plan then computes, bit for bit, what the same plan without the bit computes on the
   * dequantised float32 tables: gathers, scatters, pooled sums and means in id order from +0.0, range checks, the +0.0 rows
   * of ids outside the vocabulary.  Everything else is unchanged — the geometry, the float32 output, the blob (PASSTHROUGH /
   * BATCH_COL_REDUCTION payloads stay float32), both layouts, every id source and transform, FCP_FLAG_COUNT_BAD_IDS,
   * 2^32 - 3 rows per table; fcp_plan_table_bytes counts vocab * (dim + 8).  Plans do not quantise: they read what they
   * are given; fcp_table_convert does, once, at load time.  Together with FCP_FLAG_TABLES_BF16 / _F16: FCP_ERR_INVALID_ARGUMENT.  Refused with FCP_ERR_UNSUPPORTED:
   * together with FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16, shard_world > 1, any column with per-id weights or
   * FCP_COMBINER_SQRTN. */
  FCP_FLAG_TABLES_Q8 = 1u << 5,
  /* Per-input table formats: the format is a property of each embedding table (device input), not of the plan.  Every
   * column names its table's format in fcp_column_ext_t::table_kind1 (1 + FCP_TAB_*, 0 = float32); the field is read only
   * with this bit (`ext` NULL: every table float32).  Columns that share a table_input must name the same kind (else
   * FCP_ERR_INVALID_ARGUMENT, naming both columns); PASSTHROUGH / BATCH_COL_REDUCTION / EXTERNAL columns carry 0.  Together
   * with FCP_FLAG_TABLES_BF16 / _F16 / _Q8: FCP_ERR_INVALID_ARGUMENT.  Each table follows its own format's rules, exactly as
   * described above: layout, base alignment (4 * V | 2 * V | 2 * V | 4 bytes for float32 | bf16 | fp16 | q8), widening /
   * dequantisation; the plan computes, bit for bit, what the float32 plan computes on the widened / dequantised tables.
   * If ALL tables of the plan have one kind, the plan IS the plan-wide plan of that kind (the same kernels, the same
   * fcp_plan_last_launch, fcp_plan_table_dtype and plan-file version).  A truly mixed plan reports FCP_TAB_MIXED and its
   * kinds through fcp_plan_table_kinds; fcp_plan_table_bytes sums each table at its own row size, table shapes are checked
   * against each table's own row width.  Refused with FCP_ERR_UNSUPPORTED ("per-input table formats ..."), as the
   * plan-wide formats are: together with FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16, shard_world > 1, any column with per-id
   * weights or FCP_COMBINER_SQRTN. */
  FCP_FLAG_TABLES_PER_INPUT = 1u << 6
};
/* element type of the plan's outputs (fcp_plan_out_dtype) */
enum { FCP_OUT_F32 = 0, FCP_OUT_BF16 = 1, FCP_OUT_F16 = 2 };
/* element type of the plan's embedding tables (fcp_plan_table_dtype) */
enum { FCP_TAB_F32 = 0, FCP_TAB_BF16 = 1, FCP_TAB_F16 = 2 };
/* (FCP_FLAG_TABLES_Q8: uint8 codes with a float32 scale and bias behind every row) */
enum { FCP_TAB_Q8 = 3 };
/* (FCP_FLAG_TABLES_PER_INPUT: what fcp_plan_table_dtype answers for a plan whose tables have more than one format.  NOT a row
 * format: fcp_table_convert, fcp_table_row_bytes and fcp_table_update_rows refuse it like any other unknown kind.) */
enum { FCP_TAB_MIXED = 255 };
/* A plan without device resources: layout / arena / table-byte queries and plan-file checks on a machine
 * without a GPU (offline graph tooling).  Anything that computes returns FCP_ERR_NO_DEVICE — there is no
 * CPU fallback.  (A macro: the value does not fit an int enumerator.) */
#define FCP_FLAG_HOST_ONLY 0x80000000u

typedef struct fcp_column_desc {
  int32_t form;         /* FCP_FORM_*                                         */
  int32_t combiner;     /* FCP_COMBINER_* (form 2)                            */
  int32_t dim;          /* embedding width (table.shape[1]); form 4/5: width  */
  int32_t id_source;    /* FCP_IDS_*                                          */
  int64_t vocab;        /* table.shape[0]                                     */
  int32_t table_input;  /* index into fcp_process_args_t.input_ptrs           */
  int32_t ids_input;    /* host-input (blob tensor) index of ids / values /
                           passthrough payload                                */
  int32_t seg_input;    /* host-input index of seg ids / CSR offsets, or -1   */
  int32_t seg_kind;     /* FCP_SEG_*                                          */
  int32_t seg_stride;   /* element stride between consecutive seg ids (>=1)   */
  int32_t rows_source;  /* FCP_ROWS_*                                         */
  int32_t rows_arg;     /* symbol index / host-input index                    */
  int32_t n_boundaries; /* FCP_IDS_F32_BUCKETIZE: number of boundaries        */
  const float *boundaries; /* host pointer, copied at plan creation           */
  int32_t concat_group; /* which ConcatV2 this column feeds, 0..n_groups-1    */
  int32_t concat_slot;  /* position inside the group (ConcatOutputs
                           device_concat_indices / host_concat_indices)       */
  int32_t xform_mode;   /* FCP_XFORM_* (lookup forms only)                    */
  int32_t xform_n;      /* number of closed intervals                         */
  const int64_t *xform_lo; /* host int64[xform_n], copied at plan creation    */
  const int64_t *xform_hi;
  int64_t xform_substitute; /* FCP_XFORM_SELECT                               */
  /* > 0: categorical_column_with_hash_bucket over INTEGER ids, on the device:
   * id' = Fingerprint64(decimal string of id) % hash_buckets — what TensorFlow's
   * AsString -> StringToHashBucketFast pair computes (TF 2.6.2
   * core/kernels/string_to_hash_bucket_fast_op.h: Fingerprint64 = FarmHash
   * farmhashna::Hash64, third_party farmhash commit 816a4ae6).  Applied FIRST,
   * before the interval transform.  String features are hashed on the CPU. */
  int64_t hash_buckets;
} fcp_column_desc_t;

typedef struct fcp_plan_desc {
  int32_t abi_version;            /* FCP_ABI_VERSION                          */
  int32_t n_columns;
  const fcp_column_desc_t *columns;
  int32_t n_host_inputs;          /* ConcatInputs attr T / ranks sizes        */
  const int32_t *host_input_ranks;      /* attr "ranks"                       */
  const int32_t *host_input_elem_sizes; /* DataTypeSize of attr "T" entries   */
  int32_t n_device_inputs;        /* FeatureColumnProcess `inputs` (tables)   */
  int32_t n_groups;               /* number of concat groups                  */
  int32_t n_symbols;              /* length of the `symbols` host tensor      */
  int32_t layout;                 /* FCP_LAYOUT_*                             */
  int32_t device;                 /* HIP device ordinal                       */
  int32_t shard_rank;             /* row sharding: this GPU owns ids with     */
  int32_t shard_world;            /*   id % shard_world == shard_rank, local
                                       row id / shard_world. 1 = unsharded.   */
  uint32_t flags;                 /* FCP_FLAG_*                               */
} fcp_plan_desc_t;

typedef struct fcp_plan fcp_plan_t; /* opaque; owns const buffers on device  */

/* Allocator callback: return device memory of `bytes` bytes (or NULL).
 * Reference: std::function<void(void**,int)> malloc_temp / malloc_buff
 * (feature_column_process_op_gpu.cu.cc:99-111).  The library never frees
 * caller memory.  malloc_buff is called at most once per process call
 * (it maps to allocate_output(2)). */
typedef void *(*fcp_alloc_fn)(void *ctx, size_t bytes);

typedef struct fcp_process_args {
  const void *concated_inputs;     /* device: ConcatInputs blob (input 0)     */
  int64_t concated_bytes;
  const int32_t *concated_offsets; /* host int32[n_host_inputs]   (input 1)   */
  const int32_t *concated_shapes;  /* host int32[sum ranks]       (input 2)   */
  const void *const *input_ptrs;   /* host array of device table pointers     */
  const int32_t *input_shapes;     /* host int32[2*n_device_inputs] or NULL   */
  const int32_t *symbols;          /* host int32[n_symbols] or NULL           */
  void *stream;                    /* hipStream_t                             */
  fcp_alloc_fn malloc_temp;        /* may be NULL: plan-owned scratch is used */
  void *malloc_temp_ctx;
  fcp_alloc_fn malloc_buff;        /* required: allocates the output arena    */
  void *malloc_buff_ctx;
} fcp_process_args_t;

typedef struct fcp_process_result {
  void **output_ptrs;          /* host void*[n_columns]: device address of
                                  element (0,0) of each column's output       */
  int32_t *output_shapes;      /* host int32[2*n_columns]: rows, dim          */
  int64_t *output_row_strides; /* host int64[n_columns]: row stride, elements */
  void **group_ptrs;           /* host void*[n_groups]: concat matrices
                                  (FCP_LAYOUT_CONCAT) or NULLs                */
  int32_t *group_shapes;       /* host int32[2*n_groups]: rows, sum(dim)      */
  void *buffer;                /* the arena returned by malloc_buff           */
  int64_t buffer_bytes;
} fcp_process_result_t;

/* Plain view of a host tensor for fcp_concat_inputs. */
typedef struct fcp_host_tensor {
  const void *data;
  int32_t elem_size;
  int32_t rank;
  const int64_t *dims;
} fcp_host_tensor_t;

/* ---- library ------------------------------------------------------------- */
int fcp_abi_version(void);
const char *fcp_status_string(int status);
/* Last HIP error string seen by this thread ("" if none). */
const char *fcp_last_error(void);

/* ---- Addons>ConcatInputs (concat_inputs_ops.cc:42-77), host only --------- */
/* Sizes of the three outputs for these inputs. */
int fcp_concat_inputs_sizes(const fcp_host_tensor_t *inputs, int32_t n_inputs,
                            int64_t *blob_bytes, int32_t *rank_sum);
/* Pack: blob = byte concatenation, offsets[i] = byte offset of input i
 * (int32, as the reference), shapes = all dims in order. */
int fcp_concat_inputs(const fcp_host_tensor_t *inputs, int32_t n_inputs,
                      void *blob, int64_t blob_capacity, int32_t *offsets,
                      int32_t *shapes);

/* ---- plan: replaces code generation + CreateConstBuffers ------------------ */
int fcp_plan_create(const fcp_plan_desc_t *desc, fcp_plan_t **plan);

/* Per-column extensions (the v2 structs above stay as they are; a column without extensions is all zeros).
 *
 * Segment ids that are a FUNCTION OF SEVERAL INDEX COORDINATES — a SparseReshape between the SparseTensor and
 * the lookup, which the reference folds into the index expression of the generated code
 * (EmitInputInline, cuda_emitter.cc:1874-1916: flat index from the input shape, then / and % by the output
 * shape).  For the row coordinate of the reshaped tensor that is
 *     seg(i) = (sum_{k < seg_map_n} idx[i * seg_stride + k] * seg_map_mul[k]) / seg_map_div
 * over the first seg_map_n coordinates of element i (seg_stride = rank of the ORIGINAL indices matrix,
 * seg_kind FCP_SEG_IDS_I32/I64, form FCP_FORM_SEGMENT_REDUCE).  Factors are >= 1; one of them may additionally
 * be multiplied by a request's symbol (a dense_shape entry that is only known per request: [B, T, L] ->
 * [B*T, L] gives seg = idx0 * T + idx1): seg_map_sym >= 0 names the symbol, seg_map_sym_slot the factor
 * (0..3 = seg_map_mul[slot], 4 = seg_map_div).  seg_map_n = 0: plain segment ids, seg(i) = idx[i * seg_stride].
 * Lexicographically sorted indices (TF's SparseTensor contract) give non-decreasing seg ids. */
#define FCP_SEG_MAP_MAX 4
typedef struct fcp_column_ext {
  int32_t seg_map_n;        /* 0 = none, else 1..FCP_SEG_MAP_MAX coordinates  */
  int32_t seg_map_sym;      /* symbol index, or -1                            */
  int32_t seg_map_sym_slot; /* 0..3: seg_map_mul[slot]; 4: seg_map_div        */
  /* 1 + the host-input index of the column's per-id weights, 0 = unweighted (an all-zero record stays "no extension"):
   * float32, one per id, in the order of the ids — sp_weights of embedding_lookup_sparse / weighted_categorical_column,
   * i.e. the TF op sequence GatherV2 -> Mul(rows, weights) -> SegmentSum [-> div_no_nan by SegmentSum(weights) (mean) or
   * by Sqrt(SegmentSum(weights^2)) (sqrtn)].  Every gathered row is multiplied by its weight — a rounded product, then a
   * rounded add, never a fused multiply-add — in id order.  An id the column's FILTER drops contributes neither a term nor
   * a weight; an id outside [0, vocab) reads zeros and its weight counts in the denominator.  FCP_FORM_SEGMENT_REDUCE
   * only, any segment encoding (a folded SparseReshape included); the tensor holds exactly as many elements as the ids
   * tensor (else the request returns FCP_ERR_SHAPE_MISMATCH). */
  int32_t weights_input1;
  int64_t seg_map_mul[FCP_SEG_MAP_MAX];
  int64_t seg_map_div;
  /* FCP_FLAG_TABLES_PER_INPUT only (never read without the bit): 1 + FCP_TAB_* of the table this column reads, 0 = float32;
   * 0 for columns without a table */
  int32_t table_kind1;
  int32_t reserved0;
  int64_t reserved1[1];
} fcp_column_ext_t;
/* `ext`: NULL, or one record per column of `desc`. */
int fcp_plan_create_ex(const fcp_plan_desc_t *desc, const fcp_column_ext_t *ext, fcp_plan_t **plan);
/* The same from a column-plan FILE — what the `dlpath` attr of
 * Addons>FeatureColumnProcess names in this build (the reference dlopen()s a
 * JIT-compiled .so there, feature_column_process_op_gpu.cu.cc:49-62).  Text
 * format, written by recom_amd.plan_io.save_plan / `python -m recom_amd.graph`:
 *   fcp_plan 1 / layout L / groups G symbols S device_inputs D / host_inputs N,
 *   N lines "rank elem_size" / columns C, C lines "form combiner dim id_source
 *   vocab table_input ids_input seg_input seg_kind seg_stride rows_source
 *   rows_arg concat_group concat_slot n_boundaries b0 b1 ..." — version 2 files
 *   ("fcp_plan 2") append "xform_mode xform_n substitute hash_buckets lo0 hi0 lo1
 *   hi1 ..." to every column line; version 3 files may end with a stage section
 *   (fcp_plan_file_stage_info) that tells Addons>ConcatInputs how to pack;
 *   version 4 files may carry, before it, "segmaps M" + M lines "column n sym
 *   slot mul0 mul1 mul2 mul3 div" (fcp_column_ext_t::seg_map_*); version 5 files
 *   (plans with per-id weights or FCP_COMBINER_SQRTN) carry, before both,
 *   "weights M" + M lines "column input" (fcp_column_ext_t::weights_input1 - 1);
 *   version 6 files (narrow-output plans, and only those) carry "out_dtype bf16" or
 *   "out_dtype f16" as their SECOND line, between the header and "layout"; the line
 *   anywhere else, twice, with another name, or in a file of version <= 5 is malformed;
 *   version 7 files (plans with 16-bit tables, and only those) carry "table_dtype bf16" or
 *   "table_dtype f16" in the same place under the same rules (and no out_dtype line: the
 *   two features exclude each other); plans with 8-bit row-quantised tables are version 7
 *   files too and carry "table_dtype q8"; version 8 files (plans whose tables have more than
 *   one format, and only those) carry "table_dtypes D k0 ... k(D-1)" in that place under the
 *   same rules: one of f32 | bf16 | f16 | q8 per device input, "-" for an input no lookup
 *   column reads; plan-wide table bits in `flags` with such a file are FCP_ERR_INVALID_ARGUMENT.
 * `flags`: fcp_plan_desc_t::flags.  FCP_FLAG_OUT_BF16 / _F16 on a file without the
 * line select the dtype; bits that name the file's dtype are fine, the other dtype is
 * FCP_ERR_INVALID_ARGUMENT; FCP_FLAG_TABLES_BF16 / _F16 / _Q8 and a table_dtype line likewise.
 * FCP_ERR_INVALID_ARGUMENT for a missing or malformed file. */
int fcp_plan_create_from_file(const char *path, int32_t device, uint32_t flags,
                              fcp_plan_t **plan);
int fcp_plan_destroy(fcp_plan_t *plan);
/* Static facts: number of columns / groups / host inputs / tables / symbols
 * (any pointer may be NULL), */
int fcp_plan_counts(const fcp_plan_t *plan, int32_t *n_columns, int32_t *n_groups,
                    int32_t *n_host_inputs, int32_t *n_device_inputs,
                    int32_t *n_symbols);
/* The plan columns that are outputs of Addons>FeatureColumnProcess, in plan order
 * (every column except FCP_FORM_EXTERNAL ones): `indices` receives up to `capacity`
 * column indices, *n the count (either may be NULL). */
int fcp_plan_output_columns(const fcp_plan_t *plan, int32_t *n, int32_t *indices,
                            int32_t capacity);
/* FCP_OUT_*: the element type of the plan's outputs (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16). */
int fcp_plan_out_dtype(const fcp_plan_t *plan, int32_t *out);
/* FCP_TAB_*: the element type of the plan's embedding tables (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16 /
 * FCP_FLAG_TABLES_Q8); FCP_TAB_MIXED for a FCP_FLAG_TABLES_PER_INPUT plan whose tables have more than one format. */
int fcp_plan_table_dtype(const fcp_plan_t *plan, int32_t *out);
/* One FCP_TAB_* per device input (any plan), -1 for an input no lookup column reads: `kinds` receives up to `capacity`
 * values, *n the number of device inputs (either may be NULL). */
int fcp_plan_table_kinds(const fcp_plan_t *plan, int32_t *kinds, int32_t capacity, int32_t *n);
/* Bytes of embedding tables this plan reads on THIS device (its shard of every
 * table, shared tables counted once) and the largest single table's bytes
 * (unsharded) — the inputs of the placement gate, fcp_placement_decide; 2 bytes per
 * element in a plan with 16-bit tables, dim + 8 bytes per row in a plan with 8-bit
 * row-quantised tables, each table at its own row size in a plan with per-input formats. */
int fcp_plan_table_bytes(const fcp_plan_t *plan, int64_t *shard_bytes,
                         int64_t *max_table_bytes_unsharded);

/* ---- table conversion: writing the formats the plans read, on the device, at load time ---------------------------------- */
/* Bytes of one row of a table of `kind` (FCP_TAB_*) and width `dim`: 4 * dim | 2 * dim | 2 * dim | dim + 8 for
 * FCP_TAB_F32 | _BF16 | _F16 | _Q8; -1 for any other kind or dim <= 0.  Rows lie back to back in every format. */
int64_t fcp_table_row_bytes(int32_t kind, int32_t dim);
/* Convert `rows` rows of width `dim` between float32 and one of the compact table formats, in either direction.  `src` points
 * at the FIRST of the rows, in format src_kind; `dst` is the BASE of the destination table in format dst_kind, and the rows
 * are written at row index dst_row0 .. dst_row0 + rows - 1 (byte offset dst_row0 * fcp_table_row_bytes(dst_kind, dim), formed
 * in 64 bits).  dst_row0 lets a loader stream a checkpoint through a bounce buffer into the full compact table without forming
 * destination pointers itself: a q8 row is dim + 8 bytes, and most row addresses of a q8 table are not 4-byte aligned.
 * Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation; a plan — or any
 * other work — on the same stream sees the result.  Plans do not quantise; this entry does, once, at load time.
 *
 * Exactly one of the two kinds is FCP_TAB_F32.  Value model, so that a plan on the converted tables can be predicted bit for
 * bit:
 *   float32 -> q8    exactly the row quantized::embedding_bag_byte_prepack writes.  For a row x[0 .. dim) of finite values,
 *                    all in float32, every operation rounded once (nothing contracted): mn = min(x), mx = max(x), R = mx - mn,
 *                    scale = R / 255.0f, inv = 255.0f / (R + 1e-8f), code[i] = rint((x[i] - mn) * inv) with ties to even,
 *                    stored as a uint8; the row is the dim codes, then scale, then mn (the bias), little-endian float32.  A
 *                    constant row (R = 0) has scale 0 and codes 0.  For R > 0 the dequantised element lies within
 *                    0.5 * scale + 1e-8 + 2^-22 * max(|mn|, |mx|) of x[i].  UNSPECIFIED (but never a fault): a row with a
 *                    NaN or an infinity, a row whose R overflows float32, the sign of a zero mn in a row that holds zeros
 *                    of both signs.
 *   q8 -> float32    fma(float(code), scale, bias), rounded once: the value the plans read (FCP_FLAG_TABLES_Q8).
 *   float32 -> bf16 / fp16   fl16(x) of FCP_FLAG_OUT_BF16 / _F16: nearest-even, rounded once; overflow goes to +-inf,
 *                    underflow is gradual, -0.0 stays -0.0, NaN stays NaN (sign and payload unspecified).
 *   bf16 / fp16 -> float32   the exact widening of FCP_FLAG_TABLES_BF16 / _F16.
 * Alignment is the plan's for the same table.  With V the largest of 4 | 2 | 1 that divides dim: a float32 base is
 * 4 * V-byte aligned, a bf16 / fp16 base 2 * V-byte aligned, a q8 base 4-byte aligned; `src` obeys the rule of its own kind.
 * dst_row0 + rows stays below 2^32 - 3, the row limit of a plan's table.  The rows read and the rows written must NOT overlap;
 * this is not checked.
 *
 * Status, decided in this order (the first four need no device):
 *   FCP_ERR_INVALID_ARGUMENT  rows < 0, dst_row0 < 0, dim <= 0, a kind that is no FCP_TAB_* value, a null pointer with
 *                             rows > 0, dst_row0 + rows beyond the row limit, a misaligned dst or src, dst_kind == src_kind
 *                             (both float32, or the same compact format twice); fcp_last_error names the argument;
 *   FCP_ERR_UNSUPPORTED       two different compact formats (bf16 <-> fp16, 16-bit <-> q8): convert through float32;
 *   FCP_OK                    rows == 0: nothing is launched and no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_HIP               a kernel launch failed. */
int fcp_table_convert(void *dst, int32_t dst_kind, int64_t dst_row0, const void *src, int32_t src_kind, int64_t rows,
                      int32_t dim, int32_t device, void *stream);
/* ---- rows by id: refreshing and reading back rows of a served table --------------------------------------------------------- */
/* fcp_table_update_rows: write n float32 rows into a table of ANY format at the row indices row_ids names — the delta a
 * trainer ships to a served model.  `table` is the BASE of a table [table_rows, dim] in format `kind` (any FCP_TAB_* value,
 * float32 included: one entry for every format); `row_ids` is int64 [n] and `rows` float32 [n, dim], rows back to back, both on
 * the device.  Row i of `rows` is converted by fcp_table_convert's value model for float32 -> kind — q8: the row
 * quantized::embedding_bag_byte_prepack writes, every operation rounded once; bf16 / fp16: fl16, rounded once; float32: a copy —
 * and written at table row row_ids[i] (byte offset row_ids[i] * fcp_table_row_bytes of kind and dim, formed in 64 bits).  For
 * pairwise distinct ids the table then equals, byte for byte, what fcp_table_convert would have written from the float32
 * master with the delta applied.  Only this entry can patch a q8 row: its codes, scale and bias are the quantiser's.
 * Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation; a plan — or any
 * other work — on the same stream sees the updated rows.
 *
 * An id outside [0, table_rows) — the whole 64-bit value is compared, as the plans compare ids — is SKIPPED: its row touches
 * no memory.  `skipped` may be NULL; otherwise it points at an int64 counter on the device, which is increased by the number
 * of skipped rows (the caller zeroes it and reads it back, both on `stream`).
 *
 * The caller's side of the contract, NOT checked: the ids of one call are pairwise distinct (with duplicates the destination
 * row holds unspecified bytes — a q8 row may mix the codes of one source with the scale and bias of another — and nothing
 * outside that row is touched); `rows` and `row_ids` do not overlap the table; a request that reads the table on ANOTHER
 * stream at the same time may see either version of a row, or a q8 row of mixed parts.
 *
 * Alignment: `table` obeys the plan's rule for its kind (with V the largest of 4 | 2 | 1 that divides dim: a float32 base
 * 4 * V-byte aligned, a bf16 / fp16 base 2 * V-byte aligned, a q8 base 4-byte aligned), `rows` that of a float32 table of this
 * dim, `row_ids` and `skipped` 8 bytes.  table_rows lies in [1, 2^32 - 3), the row limit of a plan's table, and n < 2^32 - 3.
 *
 * Status, decided in this order (the first two need no device):
 *   FCP_ERR_INVALID_ARGUMENT  n < 0 or beyond its limit, table_rows outside its range, dim <= 0, a kind that is no FCP_TAB_*
 *                             value, a null table / row_ids / rows with n > 0, a misaligned pointer; fcp_last_error names
 *                             the argument between backquotes;
 *   FCP_OK                    n == 0: nothing is launched and no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
int fcp_table_update_rows(void *table, int32_t kind, int64_t table_rows, int32_t dim, const int64_t *row_ids, const float *rows,
                          int64_t n, int64_t *skipped, int32_t device, void *stream);
/* fcp_table_read_rows: the float32 values a plan reads at row_ids, for verifying an applied delta or exporting a row.  Row i of
 * `rows` (float32 [n, dim] on the device) receives table row row_ids[i] as the plans see it: fma(float(code), scale, bias)
 * rounded once for q8, the exact widening for bf16 / fp16, a copy for float32, and a row of +0.0 for an id outside
 * [0, table_rows) — the plans' rule for ids outside the vocabulary.  Bit for bit the output of a one-column FCP_FORM_GATHER
 * plan over that table.  `rows` must not overlap the table (not checked).  Arguments, alignment, limits, asynchrony and the
 * status order are those of fcp_table_update_rows. */
int fcp_table_read_rows(float *rows, const void *table, int32_t kind, int64_t table_rows, int32_t dim, const int64_t *row_ids,
                        int64_t n, int32_t device, void *stream);
/* ---- rows by id, many tables in one call: a model's delta ------------------------------------------------------------------- */
/* A model has hundreds to thousands of tables and a trainer's delta names rows in most of them; one call of the two entries
 * above per table is one device guard, one round of argument checks and one small launch per table.  fcp_tables_update_rows
 * and fcp_tables_read_rows take the whole delta: one fcp_table_rows_t per table (an ENTRY), any mix of formats and dims, and a
 * number of launches that does not grow with the number of entries.
 *
 * `entries` is a HOST array of n_tables records; it is read before the call returns and may then be freed.  Everything an entry
 * points at is on the device.  The contract is that of the single-table entries, entry by entry: after
 * fcp_tables_update_rows every byte of every table is what one fcp_table_update_rows call per entry would have left, and
 * skipped[k] (`skipped`: device int64 [n_tables], or NULL) has grown by what entry k's own call would have added to its
 * counter; fcp_tables_read_rows leaves in every entry's `rows` the bits fcp_table_read_rows leaves, a row of +0.0 for an id
 * outside the table.  Alignment, the row limit, asynchrony on `stream`, "no allocation, no synchronisation" and what is
 * unspecified (duplicate ids, overlap, a concurrent reader on another stream) are inherited unchanged.  Two entries may name
 * the same table if their ids are pairwise distinct together.
 *
 * Limits: n_tables lies in [0, 65536], and the entries of one call name at most 2^40 elements together (n * dim summed: 4 TiB
 * of float32 rows).  `workspace`: fcp_tables_rows_workspace_bytes bytes on the device, 8-byte aligned, the call's own until
 * its kernels have run (calls on one stream may share one); the size depends on n_tables alone, is a multiple of 8, does not
 * decrease with n_tables, and is -1 outside the range.
 *
 * Launches.  The entries with n > 0 are sorted into CLASSES: a q8 update by (V, G) — V the largest of 4 | 2 | 1 that divides
 * dim, G the lanes that share a row: 21 classes; every other update, and every read, by V alone: 3 classes (the format is
 * read from the entry's record, a wave-uniform branch).  A call enqueues one small launch that installs the entries' records
 * in the workspace and ONE launch per class present; a block finds its entry by a search over its class's first-block table.
 * A class of more than 2^30 threads is split as the single-table entries split their launches.  fcp_tables_rows_launches
 * (host only, no device is touched) returns the number of launches fcp_tables_update_rows enqueues for these entries, the
 * installing one included — 0 when no entry has rows, at most 25 whatever n_tables is while no class is split — computed by
 * the function the two entries build their launch list with; fcp_tables_read_rows enqueues what it returns for the same
 * entries with no q8 table among them, never more.  Invalid arguments: the negative of the status.
 *
 * Status, decided in this order (the first two need no device):
 *   FCP_ERR_INVALID_ARGUMENT  n_tables outside its range; a null `entries` with n_tables > 0; then, over the entries in
 *                             ascending order, the checks of fcp_table_update_rows in its own order and a non-zero `reserved`
 *                             (fcp_last_error reads "<entry point>: entry k: " and names the argument between backquotes);
 *                             more than 2^40 elements; a null `workspace` with n_tables > 0 or a misaligned one; a misaligned
 *                             `skipped`;
 *   FCP_OK                    n_tables == 0, or every n == 0: nothing is launched and no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_UNSUPPORTED       `stream` is capturing and there is work to do: the records are installed from the host by every
 *                             call, which a replay would not repeat (the only such case);
 *   FCP_ERR_HIP               a kernel launch failed. */
typedef struct fcp_table_rows {
  void *table;             /* base of a table [table_rows, dim] in format `kind` (any FCP_TAB_*) */
  const int64_t *row_ids;  /* device int64 [n] */
  float *rows;             /* device float32 [n, dim]: the source of an update, the destination of a read */
  int64_t table_rows, n;
  int32_t kind, dim;
  int64_t reserved[2];     /* 0 */
} fcp_table_rows_t;        /* 64 bytes */
int64_t fcp_tables_rows_workspace_bytes(int32_t n_tables);
int32_t fcp_tables_rows_launches(const fcp_table_rows_t *entries, int32_t n_tables);   /* host only */
int fcp_tables_update_rows(const fcp_table_rows_t *entries, int32_t n_tables, int64_t *skipped /* device [n_tables] or NULL */,
                           void *workspace, int32_t device, void *stream);
int fcp_tables_read_rows(const fcp_table_rows_t *entries, int32_t n_tables, void *workspace, int32_t device, void *stream);
/* ---- a delta's ids made distinct: the last occurrence of an id wins ---------------------------------------------------------- */
/* fcp_table_update_rows and fcp_table_digest_rows ask that the ids of one call be pairwise distinct and do not check.  Deltas
 * do repeat ids: two incremental checkpoints concatenated before they are applied, a parameter stream replayed after a
 * reconnect, a trainer that logs a row each time it touches it.  fcp_table_delta_distinct is the check ("is this delta
 * distinct?") and the fix ("make it distinct, the last write wins") in one entry, on the device, with neither a sort nor a lock:
 * the winner of a row is the maximum of the positions that name it, and a maximum commutes.
 *
 * `row_ids` is int64 [n] (id_bytes 8) or int32 [n] (id_bytes 4, sign-extended), as fcp_table_count_ids takes ids; `rows` is
 * float32 [n, dim], or NULL for ids only — then `rows_out` must be NULL too and `dim` is not read.  Everything is on the device.
 *
 * Who wins.  An id is inside the table when its whole 64-bit value, compared unsigned, is below table_rows (the rule of the
 * plans and of fcp_table_update_rows).  Position i WINS if its id is inside the table and no position j > i holds the same id.
 * With the winners p_0 < p_1 < ... < p_(m-1) — ascending position: the result is stable —
 *   ids_out[k]     = the id at p_k for k < m, and -1 for m <= k < n;                             int64 [n]
 *   pos_out[k]     = p_k for k < m, and -1 for m <= k < n;                                       int64 [n]; may be NULL
 *   rows_out[k, :] = the dim 32-bit words of rows[p_k, :] for k < m, copied as BITS (NaN payloads and -0.0 survive); rows
 *                    k >= m of rows_out are not touched;                                         float32 [n, dim]
 *   *report        = {n, m, duplicates, skipped}, as declared below; n == distinct + duplicates + skipped.
 * A delta that is already distinct and inside the table comes out byte for byte as it went in, with duplicates == 0: that is
 * the check.
 *
 * Chaining without the host.  The -1 tail lets (ids_out, rows_out, n) go straight into fcp_table_update_rows and
 * fcp_table_digest_rows on the same stream; no host read of m is needed.  Both skip -1 and touch no memory for it; their
 * `skipped` counters then count the n - m ids of the tail too (the delta's own ids outside the table are report->skipped).
 *
 * Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation.  `workspace` holds
 * fcp_table_delta_workspace_bytes of n bytes; its content before and after the call means nothing.  Every output byte is a
 * function of the arguments alone — not of the grid, of the hash, of the order of any atomic operation or of what the workspace
 * held: two calls leave the same bytes.  Inputs are only read; outputs must not overlap the inputs or each other (not
 * checked).  n < 2^32 - 3, and table_rows lies in [1, 2^32 - 3).  Alignment: `row_ids` id_bytes; `rows` and `rows_out` that of a
 * float32 table of this dim (4 * V bytes, V the largest of 4 | 2 | 1 that divides dim); `ids_out`, `pos_out`, `report` and
 * `workspace` 8 bytes.
 *
 * The workspace size depends on n only: a multiple of 8, non-decreasing in n, at most 40 * n + 2^20; -1 for n < 0 or n beyond
 * its limit.
 *
 * Status, decided in this order (the first needs no device), as in fcp_table_digest_rows:
 *   FCP_ERR_INVALID_ARGUMENT  n < 0 or beyond its limit; table_rows outside its range; an id_bytes that is neither 4 nor 8;
 *                             dim <= 0 with rows; a rows_out without rows, or rows without a rows_out; a null report or
 *                             workspace; a null row_ids or ids_out with n > 0; a misaligned row_ids, rows, ids_out, rows_out,
 *                             pos_out, report or workspace (in this order); fcp_last_error names the argument between backquotes;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (n == 0 included: `report` is written on the device);
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
typedef struct fcp_table_delta_report {
  int64_t n;          /* ids handed over */
  int64_t distinct;   /* rows kept: one per distinct id inside the table */
  int64_t duplicates; /* occurrences dropped because a LATER position names the same row */
  int64_t skipped;    /* ids outside [0, table_rows); n == distinct + duplicates + skipped */
} fcp_table_delta_report_t; /* 32 bytes */
int64_t fcp_table_delta_workspace_bytes(int64_t n);
int fcp_table_delta_distinct(const void *row_ids, int32_t id_bytes, const float *rows, int32_t dim, int64_t n, int64_t table_rows,
                             int64_t *ids_out, float *rows_out, int64_t *pos_out, fcp_table_delta_report_t *report, void *workspace,
                             int32_t device, void *stream);
/* ---- a model's delta made distinct: many tables in one call -------------------------------------------------------------------- */
/* fcp_tables_update_rows, fcp_tables_read_rows and fcp_tables_digest take a model's delta in one call and ask that the ids of
 * each entry be pairwise distinct; fcp_table_delta_distinct guarantees that for one table with five launches.
 * fcp_tables_delta_distinct is that entry for MANY tables: one fcp_table_delta_entry_t per table (an ENTRY), int32 and int64
 * ids, ids only and rows of any dim mixed, and a number of launches that does not grow with n_tables.
 *
 * `entries` is a HOST array of n_tables records; it is read before the call returns and may then be freed.  Everything an entry
 * points at is on the device.  Once the stream has run, for every entry k, `ids_out`, `pos_out`, the rows < m_k of `rows_out`
 * and reports[k] (`reports`: device, n_tables records) hold exactly the bytes ONE fcp_table_delta_distinct call with entry k's
 * arguments leaves; rows >= m_k of `rows_out` are not touched; an entry with n == 0 gets reports[k] = {0, 0, 0, 0} and nothing
 * else.  Entries are INDEPENDENT: each has a hash table of its own, two entries may carry the same ids, for the same table or
 * not, and an id that repeats ACROSS two entries is not seen — entries that name one table must be merged into one entry first
 * (concatenated in the order they are to be applied) if the result is to be distinct for that table.  Every output byte is a
 * function of the arguments alone: two calls leave the same bytes, whatever the workspace held.  Per entry, asynchrony on
 * `stream`, "no allocation, no synchronisation", the alignment rules, the row limit and "outputs must not overlap the inputs
 * or each other" are inherited unchanged from fcp_table_delta_distinct.
 *
 * Limits: n_tables lies in [0, 65536], and the ids of one call, n summed over its entries, stay below 2^32 - 3 (the
 * single-table limit, applied to the sum).
 *
 * `workspace`: fcp_tables_delta_workspace_bytes of the entries' n values (a host array, in entry order) bytes on the device,
 * 8-byte aligned, the call's own until its kernels have run (calls on one stream may share one); its content before and after
 * the call means nothing.  The size is a function of the n values alone: a multiple of 8, non-decreasing in every n[k], at
 * most 40 * N + 1024 * n_tables + 2^10 with N the sum of the n[k]; -1 for an invalid argument (n_tables outside its range, a
 * null n with n_tables > 0, an n[k] that is negative or beyond the limit, a sum beyond the limit).
 *
 * Launches.  One launch installs the entries' records in the workspace; then ONE clear (the entries' hash tables lie back to
 * back), ONE insert, ONE classify and ONE fold (a wave per entry) follow, whatever n_tables is, each block finding its entry
 * by a search over a first-block table; then one compact launch per CLASS present: ids only, or the (V, G) of the entry's rows
 * — V the largest of 4 | 2 | 1 that divides dim, G the lanes that share a row — 1 + 21 classes, so a call enqueues at most 27
 * launches (of the 21, the dims that exist reach 18: 24).  fcp_tables_delta_launches (host only, no device is touched) returns
 * the number for these entries, computed by the function the entry builds its launch list with: 0 for n_tables == 0, 1 when
 * every n == 0 (only the reports are written, nothing is installed), the negative of the status for invalid entries.
 * Alone, an entry takes the classify / compact grid of fcp_table_delta_distinct, B blocks (at most 1024, a block at least 1024
 * positions).  Grouped it takes that grid while the Bs of a call sum to fcp_tables_delta_deal_blocks() = 8192 or less; else
 * the grid of at most max(1, floor(B * 8192 / sum)) blocks: a call's blocks sum to at most 8192 + n_tables and no block is
 * idle.  fcp_tables_delta_grid (host only) returns the call's classify grid and, `blocks` not NULL, every entry's share (0
 * without ids).  The deal plays no part in the result.
 *
 * Status, decided in this order (the first needs no device and dereferences no device pointer):
 *   FCP_ERR_INVALID_ARGUMENT  n_tables outside [0, 65536]; a null `entries` with n_tables > 0; then, over the entries in
 *                             ascending order, what fcp_table_delta_distinct refuses for the entry's fields, in its order and
 *                             by its text (`report` and `workspace` are the call's: checked behind the entries), behind
 *                             "fcp_tables_delta_distinct: entry k: "; then 2^32 - 3 ids or more together; then a null
 *                             (n_tables > 0) or misaligned `reports`; then a null (n_tables > 0) or misaligned `workspace`;
 *   FCP_OK                    n_tables == 0: no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_UNSUPPORTED       `stream` is capturing and an entry has ids: the records are installed from the host by every
 *                             call, which a replay would not repeat (the only such case);
 *   FCP_ERR_HIP               a runtime call or a kernel launch failed. */
typedef struct fcp_table_delta_entry {
  const void *row_ids;   /* device int64 [n] (id_bytes 8) or int32 [n] (id_bytes 4) */
  const float *rows;     /* device float32 [n, dim], or NULL: ids only */
  int64_t *ids_out;      /* device int64 [n] */
  float *rows_out;       /* device float32 [n, dim]; NULL exactly when rows is NULL */
  int64_t *pos_out;      /* device int64 [n], or NULL */
  int64_t table_rows, n;
  int32_t id_bytes, dim;
} fcp_table_delta_entry_t;   /* 64 bytes */
int64_t fcp_tables_delta_workspace_bytes(const int64_t *n /* host [n_tables] */, int32_t n_tables);
int32_t fcp_tables_delta_launches(const fcp_table_delta_entry_t *entries, int32_t n_tables);  /* host only */
int32_t fcp_tables_delta_deal_blocks(void);                                                   /* host only */
int32_t fcp_tables_delta_grid(const fcp_table_delta_entry_t *entries, int32_t n_tables, int32_t *blocks /* host [n_tables] or NULL */);  /* host only */
int fcp_tables_delta_distinct(const fcp_table_delta_entry_t *entries, int32_t n_tables,
                              fcp_table_delta_report_t *reports /* device [n_tables] */,
                              void *workspace, int32_t device, void *stream);
/* ---- a new master against a served table: the rows whose stored bytes would change ------------------------------------------ */
/* Every entry above takes a delta somebody already has.  A trainer often ships a whole new float32 checkpoint instead, and a
 * digest says THAT two replicas differ, not WHERE.  fcp_table_diff turns "new rows + served table" into the delta
 * fcp_table_update_rows takes, in one pass over the new rows and the stored rows, without a temporary table, and with the
 * library's own quantiser deciding: a float32 row whose change the format cannot see — low mantissa bits that round away in
 * bf16 / fp16, a nudge far below half a code step in q8 — is not reported and need not be shipped or written.
 *
 * `table` is the BASE of a table [table_rows, dim] in format `kind` (any FCP_TAB_* value, float32 included); `src` points at the
 * FIRST of `rows` rows in format src_kind, and row i of `src` is the candidate for table row row0 + i — row0 lets a checkpoint
 * stream through a bounce buffer, as dst_row0 does for fcp_table_convert.  src_kind is FCP_TAB_F32 (the new master) or `kind`
 * (a replica of the same format: ids only, `rows_out` must be NULL); for a float32 table the two coincide and `rows_out` is
 * allowed.  Everything is on the device.
 *
 * Which rows are changed.  Table row row0 + i is CHANGED when the fcp_table_row_bytes(kind, dim) bytes fcp_table_convert
 * (float32 -> kind) writes for row i of `src` — for a replica, and for float32 against float32: the bytes of row i themselves —
 * differ in any byte from the bytes stored: a compare of BITS (-0.0 differs from +0.0, two NaNs with equal bits are
 * unchanged).  A q8 row is quantised in registers by the arithmetic of fcp_table_convert's value model and compared with the
 * stored codes and the stored scale and bias; a 16-bit row is fl16 of its elements.  Nothing is written to the table.  The answer
 * for a q8 row that holds a NaN or an infinity, or whose range overflows float32, is UNSPECIFIED (but never a fault), as its
 * bytes are in fcp_table_convert.  With the changed rows r_0 < r_1 < ... < r_(m-1) — ascending table row index —
 *   ids_out[k]     = r_k for k < m, and -1 for m <= k < rows;                                    int64 [rows]
 *   rows_out[k, :] = the dim 32-bit words of the `src` row of r_k for k < m, copied as BITS; rows k >= m of rows_out are not
 *                    touched;                                                                    float32 [rows, dim]; may be NULL
 *   *report        = {rows, m, r_0, r_(m-1)}, as declared below; -1 for both rows when m == 0.
 *
 * Chaining without the host.  The -1 tail lets (ids_out, rows_out, rows) go straight into fcp_table_update_rows and
 * fcp_table_digest_rows on the same stream; no host read of m is needed (both skip -1 and count it in their `skipped`).  After
 * that update the table's rows row0 .. row0 + rows - 1 equal, byte for byte, what fcp_table_convert of `src` at dst_row0 = row0
 * would have written.
 *
 * Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation.  `workspace` holds
 * fcp_table_diff_workspace_bytes of `rows` bytes; its content before and after the call means nothing.  Every output byte is a
 * function of the arguments alone — the grid is fixed by `rows`, one partial record per block, a one-wave fold, no atomics:
 * two calls leave the same bytes.  Inputs are only read; outputs must not overlap the inputs or each other (not checked).
 * table_rows lies in [1, 2^32 - 3), 0 <= row0 and row0 + rows <= table_rows.  Alignment: `table` and `src` obey the plan's rule
 * for their kinds (with V the largest of 4 | 2 | 1 that divides dim: float32 4 * V bytes, bf16 / fp16 2 * V bytes, q8 4 bytes),
 * `rows_out` that of a float32 table of this dim, `ids_out`, `report` and `workspace` 8 bytes.
 *
 * The workspace size depends on `rows` only — one flag byte per row and the blocks' records: a multiple of 8, non-decreasing,
 * at most rows + 2^17; -1 for rows < 0 or rows >= 2^32 - 3.
 *
 * Status, decided in this order (the first needs no device), as in fcp_table_delta_distinct:
 *   FCP_ERR_INVALID_ARGUMENT  rows < 0 or beyond its limit; table_rows outside its range; row0 < 0 or row0 + rows beyond
 *                             table_rows; dim <= 0; a kind that is no row format; a src_kind that is neither FCP_TAB_F32 nor
 *                             kind; a rows_out with a compact src_kind; a null report or workspace; a null table, src or
 *                             ids_out with rows > 0; a misaligned table, src, ids_out, rows_out, report or workspace (in this
 *                             order); fcp_last_error names the argument between backquotes;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (rows == 0 included: `report` is written on the device);
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
typedef struct fcp_table_diff_report {
  int64_t rows;          /* rows compared */
  int64_t changed;       /* rows whose stored bytes would change: m */
  int64_t first_changed; /* smallest changed table row index, -1 if none */
  int64_t last_changed;  /* largest, -1 if none */
} fcp_table_diff_report_t; /* 32 bytes */
int64_t fcp_table_diff_workspace_bytes(int64_t rows);
int fcp_table_diff(const void *table, int32_t kind, int64_t table_rows, int32_t dim, const void *src, int32_t src_kind,
                   int64_t row0, int64_t rows, int64_t *ids_out, float *rows_out, fcp_table_diff_report_t *report,
                   void *workspace, int32_t device, void *stream);
/* ---- table audit: what each compact format would do to a float32 table, before anything is written --------------------------- */
/* fcp_table_audit: judge `rows` float32 rows of width `dim` — a table before fcp_table_convert, or the rows of a delta before
 * fcp_table_update_rows — against FCP_TAB_BF16, FCP_TAB_F16 and FCP_TAB_Q8 at once, reading every source element once (the
 * part of a row beyond 256 * V elements twice, as the quantiser reads it).  fcp_table_convert and fcp_table_update_rows write
 * what they write for a row a format cannot hold (+-inf in a 16-bit table, unspecified q8 codes); this entry is how a caller
 * finds out first.  `src`, `out` and `workspace` are on the device; `workspace` holds fcp_table_audit_workspace_bytes bytes (a
 * constant, independent of rows and dim) and its content before and after the call means nothing.  Device to device on
 * `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation: `out` is read after the stream has
 * reached the call's end.
 *
 * Value model.  rt(x) is what the library itself does to an element on the way to the format and back, all in float32, every
 * operation rounded once:
 *   bf16 / fp16   the exact widening of fl16(x), fcp_table_convert's float32 -> 16-bit followed by its 16-bit -> float32;
 *   q8            fma(float(code), scale, mn) with mn, scale and code exactly as fcp_table_convert's float32 -> q8 forms them
 *                 for the row.
 * e = x - rt(x), in float32.  A row is NON-FINITE if any element is NaN or +-inf: it counts in rows_nonfinite, is bad for every
 * kind, and is not counted in any rows_bad.  A finite row is BAD for a 16-bit kind if any element rounds to +-inf (fp16:
 * |x| >= 65520), for q8 if max - min overflows float32.  A bad row is left out of that kind's error fields, a non-finite row
 * out of all sums, so no field is ever NaN.  The sums are float64 sums of exact float64 products of float32 values; their
 * order is fixed by (rows, dim), there is no atomic operation, and two calls on the same input leave the same bytes in `out`.
 * kind[FCP_TAB_F32] is zeros with first_bad_row -1.  rows == 0 is valid: zeros, and every first_* field -1.
 *
 * Alignment: `src` that of a float32 table of this dim (4 * V bytes, V the largest of 4 | 2 | 1 that divides dim); `out` and
 * `workspace` 8 bytes.  rows stays below 2^32 - 3, the row limit of a plan's table.
 *
 * Status, decided in this order (the first needs no device):
 *   FCP_ERR_INVALID_ARGUMENT  rows < 0, dim <= 0, a null out or workspace, a null src with rows > 0, rows beyond the row limit,
 *                             a misaligned pointer; fcp_last_error names the argument;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (rows == 0 included: `out` is written on the device);
 *   FCP_ERR_HIP               a kernel launch failed. */
typedef struct fcp_table_audit_kind {
  int64_t rows_bad;      /* rows this format cannot hold (non-finite rows not counted) */
  int64_t first_bad_row; /* smallest such row index, -1 if none */
  double sum_sq_err;     /* sum over good rows of (double)e * e */
  float max_abs_err;     /* max over good rows of |e| */
  int32_t reserved;      /* 0 */
} fcp_table_audit_kind_t;
typedef struct fcp_table_audit {
  int64_t rows, rows_nonfinite, first_nonfinite_row; /* a NaN or +-inf in the source; -1 if no such row */
  double sum_sq;                                     /* sum of (double)x * x over the finite rows */
  fcp_table_audit_kind_t kind[4];                    /* indexed by FCP_TAB_* */
} fcp_table_audit_t;
int64_t fcp_table_audit_workspace_bytes(void);
int fcp_table_audit(const float *src, int64_t rows, int32_t dim, fcp_table_audit_t *out, void *workspace, int32_t device,
                    void *stream);
/* fcp_table_audit_weighted: fcp_table_audit with one count per row — how often requests read the row, as fcp_table_count_ids
 * counts it.  `row_counts` is uint32 [rows] on the device.  With w_r = (double)row_counts[r] (exact) the three kinds of sums
 * become traffic-weighted: sum_sq = sum of w_r * x * x, kind[k].sum_sq_err = sum of w_r * e * e, each term added as ONE
 * fma(w_r, (double)e * (double)e, sum) — the square is exact in float64, the fused multiply-add rounds the running sum once, so
 * the sums keep the audit's bound (non-negative terms, within n * 2^-53 of the exact sum, relative, in any order).  The order is
 * the audit's own, fixed by (rows, dim), without atomics: two calls on the same input leave the same bytes, and with row_counts
 * all ones `out` is byte for byte what fcp_table_audit writes.
 * Everything that decides whether a format is ADMISSIBLE stays unweighted and equals fcp_table_audit's, field for field: rows,
 * rows_nonfinite, first_nonfinite_row and per kind rows_bad, first_bad_row and max_abs_err.  Counts are a sample: a row nobody
 * read yesterday must still not come back as +-inf tomorrow.  A row of count 0 adds +0 to the sums and still counts if it is
 * bad; a bad or non-finite row is left out of the sums whatever its count, so no field is ever NaN; reserved stays 0.
 * fcp_table_formats_choose takes such audits as they are: it minimises whatever sum_sq_err it is handed, and its default table
 * weight, 1 / sum_sq, then makes every table's relative TRAFFIC-weighted squared error count alike.
 * The struct, the workspace (fcp_table_audit_workspace_bytes), the arguments, alignment, limits, asynchrony and the status
 * order are those of fcp_table_audit; `row_counts` joins the argument checks (FCP_ERR_INVALID_ARGUMENT): null with rows > 0
 * (behind a null src), not 4-byte aligned (behind a misaligned src).  `row_counts` is only read. */
int fcp_table_audit_weighted(const float *src, int64_t rows, int32_t dim, const uint32_t *row_counts, fcp_table_audit_t *out,
                             void *workspace, int32_t device, void *stream);
/* ---- table traffic: how often requests read each row ------------------------------------------------------------------------ */
/* fcp_table_count_ids: add, to counts[r], the number of times r occurs among the `n` ids — the read counts of a table's rows,
 * taken from sampled requests, for fcp_table_audit_weighted.  `counts` is uint32 [table_rows] on the device (the caller zeroes
 * it once and may call any number of times); `ids` is int64 [n] (id_bytes 8) or int32 [n] (id_bytes 4, sign-extended) on the
 * device — the two id formats a plan's request carries, so the id inputs of a request are counted as delivered.  Accumulation
 * is modulo 2^32: the caller keeps a row below 4 G reads, or halves the array.  The ids are counted as handed over: a column
 * whose plan transforms its ids (hash, bucketize, filter, slot offset) is counted from what the caller's pipeline holds after
 * the transform.
 *
 * An id outside [0, table_rows) — the whole 64-bit value is compared, as the plans and fcp_table_update_rows compare ids —
 * touches no memory and is counted in *skipped: an int64 counter on the device, increased by the number of such ids (the caller
 * zeroes it); `skipped` may be NULL.
 *
 * Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation.  Concurrent calls
 * on other streams into the same `counts` are allowed: integer adds commute, the result is exact and independent of any order.
 * `counts` must not overlap `ids` (not checked).  Alignment: `counts` 4 bytes, `ids` id_bytes, `skipped` 8.  table_rows lies in
 * [1, 2^32 - 3), the row limit of a plan's table.
 *
 * Status, decided in this order (the first two need no device), as in fcp_table_update_rows:
 *   FCP_ERR_INVALID_ARGUMENT  n < 0, table_rows outside its range, an id_bytes that is neither 4 nor 8, a null counts or ids
 *                             with n > 0, a misaligned counts / ids / skipped; fcp_last_error names the argument between
 *                             backquotes;
 *   FCP_OK                    n == 0: nothing is launched and no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
int fcp_table_count_ids(uint32_t *counts, int64_t table_rows, const void *ids, int32_t id_bytes, int64_t n, int64_t *skipped,
                        int32_t device, void *stream);
/* ---- table traffic of a plan's request: the rows a request reads, counted through the plan's own id path ---------------------
 * fcp_table_count_ids counts ids as handed over.  Most columns of a plan do not carry row ids: they bucketize float values,
 * hash, select or filter.  These three entries count what one request — given exactly as fcp_process_feature_columns takes
 * it — reads of every table, in ONE launch, with the id path the serving kernels themselves run (decode of int32 / int64 /
 * Bucketize(float32) ids, hash, SELECT / FILTER, the 64-bit compare against the column's vocab).
 *
 * What is counted: every column of form GATHER, SEGMENT_REDUCE or GATHER_SCATTER, every position i < nnz of its id stream.
 * The transformed id is a row: counts[table_input][row] += 1.  It was dropped by the column's FILTER: nothing.  It lies
 * outside [0, vocab): no memory is touched, *skipped += 1.  This is the reference's GatherV2 — every id that reaches the
 * lookup counts once: an overwritten id or a dropped row of a scatter column counts, an id of weight 0 counts, every id of a
 * bag counts.  Columns that share a table add into one array.  On a row-sharded plan the GLOBAL row is counted, without a
 * rank filter: every rank counts what the unsharded plan would.  The table format, output dtype, layout and kernel variant
 * of the plan play no part, and the plan's own FCP_FLAG_COUNT_BAD_IDS counter is never touched.  Accumulation is modulo
 * 2^32, exact, independent of any order and safe against concurrent counts into the same arrays, as in fcp_table_count_ids.
 * Consequence: the counts equal fcp_table_count_ids applied, per column, to the column's transformed ids with table_rows =
 * the column's vocab.
 *
 * fcp_plan_table_rows: per device input the rows of the UNSHARDED table — the largest `vocab` over the lookup columns that
 * read the input (columns that share a table need not agree on it), -1 for an input no lookup column reads.  `rows`
 * receives up to `capacity` values, *n the number of device inputs (either may be NULL), as fcp_plan_table_kinds; any plan,
 * host-only ones too. */
int fcp_plan_table_rows(const fcp_plan_t *plan, int64_t *rows, int32_t capacity, int32_t *n);
/* fcp_plan_traffic_bind: counts[t] is a device uint32 [fcp_plan_table_rows()[t]] array for device input t (the caller zeroes
 * it), NULL = do not count this table; n_counts must be the plan's number of device inputs; `skipped` is a device int64 (the
 * caller zeroes it), or NULL.  The plan keeps the pointers (not the memory) until the next bind.  All counts NULL, or
 * n_counts == 0, unbinds.  The call copies to the device and may synchronise it, as binding tables may: once per sampling
 * period, not per request, and not concurrently with fcp_plan_traffic_count on the same plan.
 *   FCP_ERR_INVALID_ARGUMENT  a null plan, n_counts < 0 or neither 0 nor the number of device inputs, a null `counts` with
 *                             n_counts > 0, a counts[t] that is not 4-byte aligned, a `skipped` that is not 8-byte aligned;
 *                             fcp_last_error names the argument between backquotes;
 *   FCP_ERR_NO_DEVICE         a host-only plan (an unbind of one is FCP_OK), no usable device;
 *   FCP_ERR_HIP               an allocation or copy failed. */
int fcp_plan_traffic_bind(fcp_plan_t *plan, uint32_t *const *counts, int32_t n_counts, int64_t *skipped);
/* fcp_plan_traffic_count: count one request.  Of `args` only concated_inputs, concated_bytes, concated_offsets,
 * concated_shapes, symbols and stream are read: no table pointer, no allocator, no arena — the plan need never have served a
 * request nor bound a table.  Asynchronous on args->stream, one kernel launch, nothing for a request without ids.  The
 * request's descriptors are those fcp_process_feature_columns keeps per (shapes, stream): shapes that are resident cost
 * nothing, new shapes cost what they cost a request (and the request that follows finds them resident); no allocation on
 * this path.  Under stream capture the status is fcp_process_feature_columns' for the same residency.
 *   FCP_ERR_INVALID_ARGUMENT  null plan / args, null offsets / shapes, missing symbols, a null blob for a request with ids,
 *                             no counts bound (fcp_plan_traffic_bind);
 *   FCP_ERR_SHAPE_MISMATCH    under the conditions, and with the messages, of fcp_process_feature_columns;
 *   FCP_ERR_UNSUPPORTED       as fcp_process_feature_columns (a capture of shapes that are not resident, ...);
 *   FCP_ERR_NO_DEVICE / FCP_ERR_HIP. */
int fcp_plan_traffic_count(fcp_plan_t *plan, const fcp_process_args_t *args);
/* fcp_table_formats_choose: turn a byte budget into one format per table, from the tables' audits (copied to the host).  Host
 * only, no device.  Minimises  sum_t weight[t] * audits[t].kind[kinds_out[t]].sum_sq_err  subject to
 * sum_t rows[t] * fcp_table_row_bytes of kinds_out[t] and dims[t]  <=  budget_bytes.  table_weight NULL: 1 / sum_sq of the table
 * (0 where sum_sq is 0 or its reciprocal overflows), i.e. every table's relative squared error counts alike.  allowed_kinds: bit k admits FCP_TAB_k;
 * float32 is always admissible, a kind with rows_bad > 0 never is for that table, and a table with rows_nonfinite > 0 stays
 * float32.  The algorithm is fixed, so the answer is reproducible: per table the lower convex hull of (bytes, weighted error)
 * over its admissible kinds (equal bytes: the lower error, then the lower FCP_TAB_*; a dim-1 column thus never takes q8, 9
 * bytes against 4); every table starts at float32; hull steps are taken in increasing order of error added per byte saved
 * (ties: the lower table index) until the state fits the budget.  Every state reached minimises error + lambda * bytes for
 * some lambda, so no assignment within the bytes used has a lower error.  kinds_out[n_tables] receives the FCP_TAB_* values,
 * *bytes_out their bytes, *error_out the weighted error (either may be NULL).
 *   FCP_ERR_INVALID_ARGUMENT  a null audits / rows / dims / kinds_out with n_tables > 0, n_tables < 0, budget_bytes < 0, a
 *                             negative rows[t], dims[t] <= 0, a weight or a weighted error that is negative or not finite;
 *   FCP_ERR_UNSUPPORTED       even the smallest admissible assignment exceeds the budget; fcp_last_error names the bytes it
 *                             needs, and *bytes_out receives them. */
int fcp_table_formats_choose(const fcp_table_audit_t *audits, const int64_t *rows, const int32_t *dims, int32_t n_tables,
                             int64_t budget_bytes, uint32_t allowed_kinds, const double *table_weight, int32_t *kinds_out,
                             int64_t *bytes_out, double *error_out);
/* ---- table digest: is this table, byte for byte, the table I think it is? ------------------------------------------------------
 * fcp_table_convert, fcp_table_update_rows and a loader that streams a checkpoint through a bounce buffer all promise BYTES.
 * These entries let a deployment check the promise on the table it serves: an order-free 64-bit sum of row hashes, computed
 * where the table lies, at memory speed, for a table of any row format (FCP_TAB_F32 / _BF16 / _F16 / _Q8).
 *
 * Value model (fixed; all arithmetic unsigned, modulo 2^64).  G = 0x9e3779b97f4a7c15.  mix(x) is the 64-bit finaliser
 *   x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33      (mix(1) == 0xb456bcfc34c2cb2c).
 * With rb = fcp_table_row_bytes(kind, dim): a row is its rb bytes as stored, taken as nw = ceil(rb / 8) little-endian 64-bit words
 * w[0 .. nw), the last one zero-padded; salt = mix(((uint64)(kind + 1) << 32) | (uint32)dim); the hash of the row with GLOBAL
 * index r is
 *   H(r) = mix(salt + (r + 1) * G + sum over j of mix(w[j] ^ ((j + 1) * G)))
 * and the digest of a set of rows is the sum of their H.  Local row i of the rows handed over has global index
 * row0 + i * row_step.  So the digest depends on every byte and on where it lies (which word, which row, which kind and dim),
 * and on nothing else: no order of summation, grid shape or chunking can change it.  Consequences:
 *   sharding   rank g of a table row-sharded id % world (local row id / world) passes row0 = g, row_step = world: the ranks'
 *              digests add up to the digest of the unsharded table;
 *   chunking   a checkpoint digested chunk by chunk (row0 = the chunk's first row) adds up to the digest of the whole table;
 *   deltas     new digest = old digest - (digest of the touched rows before) + (digest of the same rows after): a digest is
 *              maintained across fcp_table_update_rows from the touched rows alone (fcp_table_digest_rows).
 * The digest detects ACCIDENTS: a changed byte, swapped rows, swapped words, a row at the wrong index, the same bytes read as
 * another kind or dim.  It is NOT a MAC and no cryptographic hash: whoever can choose the bytes can choose the sum.
 *
 * fcp_table_digest: the digest of `rows` rows that lie back to back from `first_row` — the table's base or ANY row of it, so
 * that a range of rows or one chunk of a bounce buffer can be digested.  `first_row`, `out` and `workspace` are on the device;
 * `workspace` holds fcp_table_digest_workspace_bytes bytes (a constant) and its content before and after the call means
 * nothing.  Device to device on `device`, asynchronous on `stream` (a hipStream_t), no allocation, no synchronisation; no
 * atomic operation, and two calls on the same input leave the same bytes.  Once the stream has run, `out` is
 * {sum, rows, 0, 0}; rows == 0 gives zeros.  The table is only read, and no load touches a byte outside
 * [first_row, first_row + rows * rb): the partial last word of a row is read with loads that stay inside the row.
 * Alignment: `first_row` that of a row of the kind — 4 * V bytes for float32, 2 * V for bf16 / fp16, V the largest of 4 | 2 | 1
 * that divides dim; ANY byte address for q8, whose rows of dim + 8 bytes start anywhere; `out` and `workspace` 8 bytes.  rows
 * stays below 2^32 - 3, the row limit of a plan's table, and a row below 2 GiB.
 *
 * Status, decided in this order (the first needs no device):
 *   FCP_ERR_INVALID_ARGUMENT  rows < 0 or beyond the row limit; dim <= 0; a kind that is no FCP_TAB_* row format; row0 < 0;
 *                             row_step < 1; row0 + (rows - 1) * row_step overflowing int64; a null out or workspace; a null
 *                             first_row with rows > 0; a misaligned first_row, out or workspace (in this order);
 *                             fcp_last_error names the argument between backquotes;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (rows == 0 included: `out` is written on the device);
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
typedef struct fcp_table_digest {
  uint64_t sum;     /* the digest: sum of H over the rows, modulo 2^64 */
  int64_t rows;     /* rows that were summed */
  int64_t skipped;  /* fcp_table_digest_rows: ids outside [0, table_rows); else 0 */
  int64_t reserved; /* 0 */
} fcp_table_digest_t; /* 32 bytes */
int64_t fcp_table_digest_workspace_bytes(void);
int fcp_table_digest(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step,
                     fcp_table_digest_t *out, void *workspace, int32_t device, void *stream);
/* fcp_table_digest_rows: the same sum over the rows `row_ids` names — int64 [n] on the device — of a table [table_rows, dim]
 * whose BASE is `table`.  An id in [0, table_rows) adds H(row0 + id * row_step) of that row and counts in out->rows; any other
 * id — the whole 64-bit value is compared, as fcp_table_update_rows compares ids — touches no memory, adds nothing and counts
 * in out->skipped.  An id is summed as often as it occurs.  Delta bookkeeping (digest - before + after around
 * fcp_table_update_rows) therefore needs the ids of one call pairwise distinct, as fcp_table_update_rows itself does; this is
 * NOT checked.  The sum over the ids 0 .. table_rows - 1 is fcp_table_digest of the table.  Workspace, asynchrony and
 * alignment are those of fcp_table_digest (`table` as first_row; `row_ids` 8 bytes); table_rows lies in [0, 2^32 - 3) and
 * n < 2^32 - 3.
 *
 * Status, decided in this order (the first needs no device):
 *   FCP_ERR_INVALID_ARGUMENT  n < 0 or beyond its limit; table_rows outside its range; dim <= 0; a kind that is no FCP_TAB_*
 *                             row format; row0 < 0; row_step < 1; row0 + (table_rows - 1) * row_step overflowing int64; a
 *                             null out or workspace; a null table with n > 0 and table_rows > 0; a null row_ids with n > 0; a
 *                             misaligned table, row_ids, out or workspace (in this order); fcp_last_error names the argument
 *                             between backquotes;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (n == 0 included: `out` is written on the device);
 *   FCP_ERR_HIP               a kernel launch failed.
 * No combination of valid arguments is FCP_ERR_UNSUPPORTED. */
int fcp_table_digest_rows(const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step,
                          const int64_t *row_ids, int64_t n, fcp_table_digest_t *out, void *workspace, int32_t device, void *stream);
/* fcp_table_digest_host: the same value from HOST memory — a checkpoint before it is loaded, a table copied back.  Host only:
 * it never touches a device.  Rows may start at any byte.  Returns 0 for invalid arguments (those of fcp_table_digest without
 * out and workspace), which is also the digest of no rows. */
uint64_t fcp_table_digest_host(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step);
/* ---- grouped digest: a model's tables, or a delta's rows in all of them, in one call ------------------------------------------ */
/* fcp_tables_digest is fcp_table_digest and fcp_table_digest_rows for MANY tables: one fcp_table_digest_entry_t per table (an
 * ENTRY), any mix of formats, dims and of the two modes, and a number of launches that does not grow with n_tables.  Once the
 * stream has run, out[k] holds exactly the 32 bytes ONE call would have left for entry k — fcp_table_digest when its row_ids is
 * NULL, fcp_table_digest_rows otherwise — `rows`, `skipped` and `reserved == 0` included; an entry with nothing to sum leaves
 * zeros.  The value model is the one above.  Everything the single entries promise is inherited: no atomics, two calls leave the
 * same bytes, no load touches a byte outside an entry's rows, q8 rows start at any byte, the alignment rules per kind, the row
 * limits; asynchronous on `stream`, no allocation, no synchronisation.  Entries may alias (chunks of one table, the same table
 * twice); tables are only read.
 *
 * `entries` is a HOST array of n_tables entries, n_tables in [0, 65536], read before the call returns.  `out` (n_tables records)
 * and `workspace` (fcp_tables_digest_workspace_bytes of n_tables bytes; its content before and after the call means nothing,
 * and it is the call's own until the stream has passed the call) are on the device, 8-byte aligned.  The workspace size
 * depends on n_tables alone: a multiple of 8, non-decreasing, -1 outside the range.
 *
 * Launches.  An entry with rows belongs to the class (A, G, by-id) of the digest kernel it would run alone: A the largest
 * power of two up to 8 that divides the entry's address and its row bytes, G the lanes that share a row (the largest power
 * of two not above the row's 64-bit words, at most 64), by-id whether row_ids is set — 56 classes, none folded.  A call enqueues
 * one upload, one launch per class PRESENT (a fixed order; entries inside a class in ascending order) and one fold: at most 58
 * launches whatever n_tables is.  fcp_tables_digest_launches returns that number for the same arguments — 0 for n_tables ==
 * 0, the negative status for invalid ones — from the function fcp_tables_digest builds its launch list with; host only.
 * Alone, an entry of `count` rows (ids) takes B = min(2048, ceil(count / (256 / G))) blocks.  Grouped it takes at most that, at
 * least 1 when it has rows: exactly B while the Bs of a call sum to 8192 or less, else max(1, floor(B * 8192 / sum)) — so
 * the blocks of a call sum to at most 8192 + n_tables, and a single-entry call takes the single-table grid.  `blocks`, if
 * not NULL, receives every entry's share (0 without rows).  The deal plays no part in the result: the sums are integers.
 *
 * Stream capture: a call with n_tables > 0 installs its records from the host (a pinned ring and an upload kernel, as
 * fcp_tables_update_rows does), which a replay would not repeat: FCP_ERR_UNSUPPORTED while `stream` is capturing.
 *
 * Status, decided in this order (the first needs no device and dereferences no device pointer):
 *   FCP_ERR_INVALID_ARGUMENT  n_tables outside [0, 65536]; a null `entries` with n_tables > 0; then, over the entries in
 *                             ascending order, what the matching single-table entry refuses for the entry's fields, in its
 *                             order (`table` is its first_row / table, `rows` its rows / table_rows), then a non-zero
 *                             `reserved`, then n != 0 with a null row_ids; then a null (n_tables > 0) or misaligned `out`;
 *                             then a null (n_tables > 0) or misaligned `workspace`.  fcp_last_error names the argument
 *                             between backquotes, behind "fcp_tables_digest: entry k: " for an entry's;
 *   FCP_OK                    n_tables == 0: no device is touched;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device;
 *   FCP_ERR_UNSUPPORTED       `stream` is capturing — the only case;
 *   FCP_ERR_HIP               a runtime call or a kernel launch failed. */
typedef struct fcp_table_digest_entry {
  const void *table;        /* row_ids == NULL: the first of `rows` rows lying back to back (fcp_table_digest's first_row);
                               else the table's BASE (fcp_table_digest_rows' table) */
  const int64_t *row_ids;   /* device int64 [n], or NULL */
  int64_t rows;             /* row_ids == NULL: rows to digest; else table_rows */
  int64_t n;                /* ids; 0 when row_ids == NULL */
  int64_t row0, row_step;
  int32_t kind, dim;
  int64_t reserved;         /* 0 */
} fcp_table_digest_entry_t; /* 64 bytes */
int64_t fcp_tables_digest_workspace_bytes(int32_t n_tables);
int32_t fcp_tables_digest_launches(const fcp_table_digest_entry_t *entries, int32_t n_tables, int32_t *blocks /* host [n_tables] or NULL */);  /* host only */
int fcp_tables_digest(const fcp_table_digest_entry_t *entries, int32_t n_tables, fcp_table_digest_t *out /* device [n_tables] */,
                      void *workspace, int32_t device, void *stream);
/* ---- outputs compare: what two requests' outputs differ by, per column ------------------------------------------------------- */
/* The audits predict what a table ROW loses in a format.  fcp_outputs_compare measures what a request's OUTPUT lost: two plans —
 * float32 tables and the formats fcp_table_formats_choose picked, a plan before and after a delta, two kernel variants — serve
 * the same request into two arenas, and this one call, in stream order behind them, leaves one record per column and one for
 * all columns together.  It answers: which column moved and by how much, is the output bit for bit what it was, does it hold
 * NaN or +-inf.  In pooled columns the errors of a bag's rows add up or cancel, and a narrow output rounds once more: neither
 * shows in an audit.
 *
 * `ptrs_*`, `row_strides_*` (in elements) and `shapes` (rows, dim per column) are HOST arrays of n_columns entries (shapes: 2 *
 * n_columns), exactly what fcp_process_result_t carries as output_ptrs, output_row_strides and output_shapes: a side's columns
 * may lie in a concat matrix (stride = the group's width) or in the per-column layout (stride = dim), the two sides may differ
 * in strides, layout and element kind, and they share `shapes`.  out_kind_* is FCP_OUT_F32, FCP_OUT_BF16 or FCP_OUT_F16, the
 * element kind of that side's plan; all nine pairs are served.  The arrays are read before the call returns and may be freed
 * then.  A side that is the result of a private-stream request is waited for on `stream`, as fcp_concat_outputs does.
 *
 * Value model.  A 16-bit element is widened to float32 exactly (as the plans read 16-bit tables).  For a pair (a, b) of
 * column k — element (row, j) of side A and of side B:
 *   differ     the float32 bit patterns differ: +0 against -0 differs, a NaN against the same NaN does not;
 *   finite     neither a nor b is NaN or +-inf.  A non-finite pair counts in `nonfinite` (and in `differ` and
 *              first_differ_row if its patterns differ) and enters no sum and no maximum, so no field is ever NaN;
 *   e = b - a  ONE float32 subtraction (it may overflow to +-inf: max_abs_err and sum_sq_err are then +inf); (double)e * e
 *              and (double)a * a are exact, each is added to its float64 sum by one fused multiply-add; |e| and |a| join
 *              float32 maxima.
 * Denormals are kept, every operation rounds once.  The sums' order is fixed by (shapes, n_columns, the alignment of strides
 * and pointers); there is no atomic operation, and two calls on the same input leave the same bytes in `out`.  A float64 sum
 * of n non-negative terms lies within n * 2^-53 of the exact sum, relative, in any order.
 *
 * out[k], k < n_columns, is column k's record; out[n_columns] is the record of all columns together: counts and sums of the
 * column records folded in one fixed order (a function of n_columns alone), the maxima joined, first_differ_row the smallest
 * of the columns'.  A column with rows == 0 gets zeros with first_differ_row -1; n_columns == 0 writes that one record.
 * `out` (n_columns + 1 records) and `workspace` (fcp_outputs_compare_workspace_bytes of n_columns bytes; its content before
 * and after the call means nothing) are on the device, 8-byte aligned.  Asynchronous on `stream` (a hipStream_t), no
 * allocation on the device, no synchronisation: `out` is read after the stream has reached the call's end.  Both arenas are
 * only read.  Concurrent calls with workspaces of their own are allowed.
 *
 * The workspace size depends on n_columns alone: a multiple of 8, non-decreasing, -1 for a negative argument.
 *
 * Stream capture: a call with n_columns > 0 installs its column descriptors from the host (a pinned ring and an upload kernel,
 * as the request path installs shapes that are not resident), which a replay would not repeat: FCP_ERR_UNSUPPORTED while
 * `stream` is capturing.  n_columns == 0 installs nothing and may be captured.
 *
 * Status, decided in this order (none of the first group needs a device or dereferences a column pointer):
 *   FCP_ERR_INVALID_ARGUMENT  with n_columns != 0, a null ptrs_a, row_strides_a, ptrs_b, row_strides_b or shapes (in this
 *                             order); an out_kind_a, then an out_kind_b, that is no FCP_OUT_* kind; n_columns < 0; then, each
 *                             over the columns in ascending order: negative rows or dim <= 0; a row_strides_a, then a
 *                             row_strides_b, below dim; a null ptrs_a[k], then ptrs_b[k], where rows > 0; a ptrs_a[k], then
 *                             ptrs_b[k], not aligned to its element size; then a null out, a null workspace, a misaligned
 *                             out, a misaligned workspace.  (rows at or above 2^32 - 3, the plans' row limit, would follow:
 *                             int32 shapes cannot hold such a value.)  fcp_last_error names the argument between backquotes
 *                             and, for the per-column conditions, the column;
 *   FCP_ERR_NO_DEVICE         no usable gfx950 device (n_columns == 0 included: `out` is written on the device);
 *   FCP_ERR_UNSUPPORTED       n_columns > 0 on a capturing stream — the only case;
 *   FCP_ERR_HIP               a runtime call or a kernel launch failed. */
typedef struct fcp_output_error {
  int64_t elems;            /* rows * dim pairs of this column */
  int64_t differ;           /* pairs whose float32 bit patterns (after exact widening of 16-bit elements) differ */
  int64_t nonfinite;        /* pairs in which a or b is NaN or +-inf: they enter no sum and no maximum */
  int64_t first_differ_row; /* smallest row holding a differing pair, -1: none */
  double sum_sq_ref;        /* sum of a*a over the finite pairs */
  double sum_sq_err;        /* sum of e*e, e = b - a in float32 (one rounding), over the finite pairs */
  float max_abs_err;        /* largest |e| over the finite pairs, 0 if none */
  float max_abs_ref;        /* largest |a| over the finite pairs, 0 if none */
  int64_t reserved;         /* 0 */
} fcp_output_error_t; /* 64 bytes */
int64_t fcp_outputs_compare_workspace_bytes(int32_t n_columns);
int fcp_outputs_compare(const void *const *ptrs_a, const int64_t *row_strides_a, int32_t out_kind_a, const void *const *ptrs_b,
                        const int64_t *row_strides_b, int32_t out_kind_b,
                        const int32_t *shapes /* host int32[2*n_columns]: rows, dim */, int32_t n_columns,
                        fcp_output_error_t *out /* device [n_columns + 1] */, void *workspace, int32_t device, void *stream);
/* ---- placement gate (replaces check_table_size, cuda_emitter.cc:1080-1094) -------- */
/* The reference keeps a column on the CPU when its table exceeds max_table_size =
 * 256 MiB (fc_optimize_pass.cc:71, RECOM_CPU_GPU_CO_RUN).  On MI355X the question is
 * whether the model's tables fit ONE GPU's HBM: if they do, every GPU serves requests
 * on its own replica and nothing is exchanged; only when the aggregate exceeds one
 * GPU are the tables sharded over the `world` GPUs of the node, by whole columns
 * (final blocks exchanged, bit-identical results; needs every table to fit one GPU)
 * or by rows (partial sums exchanged + fcp_shard_finalize; any table size). */
enum {
  FCP_PLACE_REPLICATE = 0,
  FCP_PLACE_COLUMN_SHARD = 1,
  FCP_PLACE_ROW_SHARD = 2,
  /* whole tables wherever a table fits one GPU, rows only for the tables that do not: the fewest bytes on the wire
   * (a whole column sends its FINAL block, 1/world of a row-sharded column's dense partial sums).  As a preference
   * (prefer_mode) it resolves to COLUMN_SHARD when every table fits, to MIXED when some do not, and falls back to
   * ROW_SHARD when whole tables cannot be packed or fewer tables than ranks would stay whole (the whole-column step
   * gives every rank a block). */
  FCP_PLACE_MIXED = 3
};
typedef struct fcp_placement {
  int32_t mode;          /* FCP_PLACE_*                                        */
  int32_t min_world;     /* fewest GPUs on which the tables fit at all          */
  int64_t bytes_per_gpu; /* table bytes the fullest GPU holds under `mode`      */
} fcp_placement_t;
/* table_bytes[n_tables]: bytes of every (unsharded) table; hbm_bytes: one GPU's
 * memory; reserve_bytes: what must stay free (arenas, request blobs, runtime);
 * prefer_mode: FCP_PLACE_COLUMN_SHARD or FCP_PLACE_ROW_SHARD, taken when both are
 * feasible, or FCP_PLACE_MIXED.  FCP_ERR_UNSUPPORTED (with min_world set) when the
 * tables do not fit `world` GPUs. */
int fcp_placement_decide(const int64_t *table_bytes, int32_t n_tables,
                         int64_t hbm_bytes, int64_t reserve_bytes, int32_t world,
                         int32_t prefer_mode, fcp_placement_t *out);
/* The same decision with the assignment: owner[t] = the rank that holds table t whole, or -1 = its rows are spread over
 * all ranks (every table under ROW_SHARD; under MIXED only the tables larger than one GPU's budget), or 0 under
 * REPLICATE (every rank holds everything).  Whole tables are dealt longest-first onto the least loaded rank, on top of
 * the row shares every rank holds. */
int fcp_placement_assign(const int64_t *table_bytes, int32_t n_tables,
                         int64_t hbm_bytes, int64_t reserve_bytes, int32_t world,
                         int32_t prefer_mode, int32_t *owner, fcp_placement_t *out);

/* total concat width of a group (sum of dims in slot order)
 * and the element offset of a column inside its group. */
int fcp_plan_group_width(const fcp_plan_t *plan, int32_t group, int32_t *width);
int fcp_plan_column_offset(const fcp_plan_t *plan, int32_t column,
                           int32_t *offset);
/* Arena bytes ProcessFeatureColumns will request for these run-time shapes
 * (buffer_size_sum, cuda_emitter.cc:2151-2158). */
int fcp_plan_arena_bytes(fcp_plan_t *plan, const int32_t *concated_shapes,
                         const int32_t *symbols, int64_t *bytes);
/* Device error counter (FCP_FLAG_COUNT_BAD_IDS); synchronises `stream`. */
int fcp_plan_read_bad_ids(fcp_plan_t *plan, void *stream, int64_t *count);

/* ---- diagnostics: what the last request launched (read-only) ------------------------------------------------------------
 * The kernel variant, block counts and output store policy of the plan's most recent fcp_process_feature_columns (or
 * the request of fcp_shard_step_run) — so a test can assert which instantiation it reached.  The request path records
 * it with relaxed stores and no lock: while host threads issue requests on the plan concurrently the fields may come
 * from different requests.  Before the first request: kernel FCP_LAUNCH_NONE, and zero block counts. */
enum {
  FCP_LAUNCH_NONE = 0, FCP_LAUNCH_DENSE = 1, FCP_LAUNCH_RAGGED = 2, FCP_LAUNCH_HYBRID = 3,
  /* the ragged body with per-id weights and the sqrtn combiner: every span of a plan that has a weighted or SQRTN column */
  FCP_LAUNCH_RAGGED_WEIGHTED = 4,
  /* the narrow-output instantiations of the three (FCP_FLAG_OUT_BF16 / FCP_FLAG_OUT_F16 plans) */
  FCP_LAUNCH_DENSE_NARROW = 5, FCP_LAUNCH_RAGGED_NARROW = 6, FCP_LAUNCH_HYBRID_NARROW = 7,
  /* the 16-bit-table instantiations of the three (FCP_FLAG_TABLES_BF16 / FCP_FLAG_TABLES_F16 plans) */
  FCP_LAUNCH_DENSE_TAB16 = 8, FCP_LAUNCH_RAGGED_TAB16 = 9, FCP_LAUNCH_HYBRID_TAB16 = 10,
  /* the 8-bit row-quantised-table instantiations of the three (FCP_FLAG_TABLES_Q8 plans) */
  FCP_LAUNCH_DENSE_TABQ8 = 11, FCP_LAUNCH_RAGGED_TABQ8 = 12, FCP_LAUNCH_HYBRID_TABQ8 = 13,
  /* the per-input-format instantiations of the three (FCP_FLAG_TABLES_PER_INPUT plans whose tables really differ) */
  FCP_LAUNCH_DENSE_TABMIX = 14, FCP_LAUNCH_RAGGED_TABMIX = 15, FCP_LAUNCH_HYBRID_TABMIX = 16
};
/* (FCP_LAUNCH_STORE_SC1: write-through without the streaming hint, a form of the plain dense kernel alone) */
enum { FCP_LAUNCH_STORE_NT = 0, FCP_LAUNCH_STORE_SC1_NT = 1, FCP_LAUNCH_STORE_PLAIN = 4, FCP_LAUNCH_STORE_SC1 = 8 };
enum { FCP_LAUNCH_SEG_NONE = 0, FCP_LAUNCH_SEG_PREPASS = 1, FCP_LAUNCH_SEG_SEARCH = 2 };
typedef struct fcp_launch_info {
  int32_t kernel;           /* FCP_LAUNCH_*: no kernel (empty request), dense, ragged, the hybrid of the two, or the weighted ragged kernel */
  int32_t vec;              /* floats per slot (V of the instantiation): the gcd of the plan's column dims, 1 | 2 | 4 */
  int32_t rows_per_wave;    /* dense body (R of the instantiation): 1 | 2 | 4 */
  int32_t store_policy;     /* FCP_LAUNCH_STORE_*: output stores `nt`, write-through `sc1 nt`, plain, or `sc1` */
  int32_t wide_rows;        /* 1: 64-bit row arithmetic in the dense body (a table shard of >= 2^32 - 3 slots) */
  int32_t shard_world;      /* > 1: the SHARDED instantiation (row-sharded plan) */
  int32_t dense_blocks;     /* blocks of the dense body (0: none) */
  int32_t ragged_blocks;    /* blocks of the ragged body (0: none) */
  int32_t segment_offsets;  /* FCP_LAUNCH_SEG_*: segment-id columns took the pre-pass kernel, or the blocks searched */
} fcp_launch_info_t;
int fcp_plan_last_launch(const fcp_plan_t *plan, fcp_launch_info_t *out);
/* Which front the dense kernel of the plan's most recent request had: the generic one (fcp_dense_kernel and its hybrid /
 * narrow forms) or the plain one (fcp_dense_kernel_plain: float32 concat plans of one group whose columns are all plain
 * gathers, requests of at least 64 rows; FCP_DIAG=dense_generic at plan creation keeps such a plan on the generic kernel).
 * fcp_plan_last_launch reports FCP_LAUNCH_DENSE, V 4, R 4 and the same grid for both.  Relaxed stores, as there. */
enum { FCP_DENSE_FRONT_NONE = 0, FCP_DENSE_FRONT_GENERIC = 1, FCP_DENSE_FRONT_PLAIN = 2 };
int fcp_plan_last_dense_front(const fcp_plan_t *plan, int32_t *front);
/* Where the plan's most recent request put its segment-offset scratch (the pre-pass's CSR offsets, or the inverse map of
 * an any-order ScatterNd column): *csr_arena_off = its byte offset in the request's arena (-1 before the first request),
 * csr_base[k] = the int32 index of column k's range inside it, or -1 for a column without one (k < capacity; either
 * pointer may be NULL).  Relaxed stores, as fcp_plan_last_launch. */
int fcp_plan_last_csr(const fcp_plan_t *plan, int64_t *csr_arena_off, int32_t *csr_base, int32_t capacity);
/* Process-wide launch counters of the kernels outside the fused matrix, one per instantiation (relaxed atomics: the
 * stager's copies are enqueued from pack-pool threads).  counts[i] for i < min(capacity, FCP_AUX_KERNELS), in the order
 * of the enum; `reset`: zero them after reading.  Returns FCP_AUX_KERNELS, or a negative status. */
enum {
  FCP_AUX_SEGMENT_OFFSETS = 0, /* the pre-pass: fcp_segment_offsets_kernel          */
  FCP_AUX_SHARD_FINALIZE_V4 = 1, FCP_AUX_SHARD_FINALIZE_V2 = 2, FCP_AUX_SHARD_FINALIZE_V1 = 3,
  FCP_AUX_CONCAT_V4 = 4, FCP_AUX_CONCAT_V2 = 5, FCP_AUX_CONCAT_V1 = 6,
  FCP_AUX_UPLOAD = 7,          /* descriptor upload: fcp_upload_kernel              */
  FCP_AUX_H2D_COPY = 8,        /* the request stager's copy: fcp_h2d_copy_kernel   */
  FCP_AUX_KERNELS = 9
};
int fcp_aux_launch_counts(int64_t *counts, int32_t capacity, int32_t reset);

/* ---- ProcessFeatureColumns (cuda_emitter.cc:2303-2494) ------------------- */
/* HIP graphs: a request whose shapes are resident (it ran once on this stream) only
 * enqueues kernels, so the call may be made while `stream` is being captured.  The
 * recorded launch reads the request's descriptor slot whenever the graph is replayed:
 * the slot is then kept until fcp_plan_release_captures (call it once the graphs are
 * destroyed).  Capturing a request whose shapes are NOT resident returns
 * FCP_ERR_UNSUPPORTED (descriptors cannot be installed inside a capture), as does a
 * request with new shapes once all 8 slots belong to captured graphs — a plan serves
 * at most 8 captured shapes at a time — and a request whose tables are not bound to
 * the plan yet, or have moved (binding copies records and may synchronise the device).
 * fcp_shard_finalize follows the same rules. */
int fcp_plan_release_captures(fcp_plan_t *plan);
int fcp_process_feature_columns(fcp_plan_t *plan,
                                const fcp_process_args_t *args,
                                fcp_process_result_t *result);

/* ---- plan-owned private streams: overlap behind ONE caller stream (EXPERIMENTAL: opt-in, frozen since round 5; the default
 * request path never enters it; recom_amd/csrc/fcp_lanes.hip) ---------- */
/* TensorFlow hands a GPU op exactly one compute stream
 * (feature_column_process_op_gpu.cu.cc:65-131 takes it from the op context; the
 * serve workers of the reference harness share one Session and therefore that one
 * stream, examples/cc/recom_examples.patch:193-216).  On one stream every request
 * pays its own kernel boundary, dependent front and drain; requests on
 * neighbouring streams hide them (S2, batch 512: ~28.5 us alone, ~23 us
 * overlapped).  fcp_plan_set_private_streams(plan, n, flags) gives the plan n
 * streams of its own (0 = off, the default; at most 16).  From then on
 * fcp_process_feature_columns
 *   - calls malloc_buff, THEN records an event on args->stream (everything
 *     enqueued there up to the allocation: the producer of the blob, and whatever
 *     still uses the memory malloc_buff has just handed out — TF's allocator reuses
 *     memory in compute-stream order, and another Session::Run thread may queue a
 *     reader of that memory at any time before the allocation),
 *   - runs the request on the next private stream (round robin), which waits for
 *     that event before its first command that touches the arena,
 *   - files the request's completion event under the address range of its arena
 *     (fcp_process_result_t::buffer, buffer_bytes).
 * args->stream itself does NOT wait for the kernels.  Whoever reads the arena —
 * Addons>ConcatOutputs in the rewritten graph, whose `tensor_buffers` inputs keep
 * blob, tables and arena alive until then (cuda_emitter.cc:2632-2643) — calls
 * fcp_result_wait(pointer into the arena, its stream) before it enqueues the
 * reader: a device-side wait, the host never blocks.  fcp_result_synchronize is
 * the same for a host reader.  Both return FCP_OK at once when nothing is pending
 * for that address (private streams off, or the request long complete).
 * fcp_concat_outputs_host performs the wait itself for its `out` pointer, fcp_concat_outputs and the
 * scatter variants for EVERY input (columns of one arena or of several) and for `out`.
 *
 * FCP_PRIVATE_NO_CALLER_WAIT: the private stream does not wait for args->stream.
 * Only for callers that guarantee by other means that the blob is complete and
 * that nothing still enqueued on their stream touches the arena memory (a
 * harness with its own arena ring); never under TensorFlow's allocator.
 * Requests issued while args->stream is being captured into a HIP graph stay on
 * args->stream.  Call it while no request of the plan is in flight (normally
 * right after plan creation); changing the count synchronises the old streams.
 * The sharded step (fcp_shard_step_run) always runs on args->stream.
 *
 * When the mode pays (round 5, profiles/r05_caller_threads_grid.txt): only when
 * the READER of a request is queued on args->stream at least one other request
 * later — every request waits for everything recorded on args->stream before its
 * allocation, readers included, so a reader right behind its request (what one
 * Session::Run of the rewritten graph does: FeatureColumnProcess, then
 * ConcatOutputs) serialises the requests again and the events are pure cost (S2
 * 30 -> 36-39 us, with 1 to 4 host threads on the stream); two requests behind:
 * 30.1 -> 24.7-25.3 us.  The supervisor below demotes callers for whom it does
 * not pay.
 *
 * Which requests take a private stream: the cross-stream events cost the host
 * about 8 us per request, so a request only gains when its kernel is long enough
 * to have something to overlap (S2 28 -> 24.5 us, RAGGED 27.8 -> 22 us per
 * request; the reference's models E / F, 10 us kernels, LOSE: 10 -> 16 us).  The
 * plan therefore keeps requests whose work — table rows gathered + output bytes
 * of the shapes it installed last — is below 48 MiB on args->stream
 * (FCP_PRIVATE_MIN_WORK_BYTES overrides); FCP_PRIVATE_ALWAYS sends every request
 * to a private stream.  Three streams measured best (two: 25-27 us on S2); with
 * four or more event-linked streams in flight every request took 35-100 us, so
 * at most three are used whatever n_streams says (the call still succeeds) — and
 * the streams belong to the DEVICE, not to the plan: every plan of the process on
 * that GPU rotates over the same three (two models with streams of their own
 * would be six event-linked queues).  They live as long as the process.
 *
 * Verification.  Whether event-linked streams overlap on the GPU depends on which
 * hardware queues the HIP runtime mapped them to — the creation order of every
 * stream of the process, GPU_MAX_HW_QUEUES, stream priorities — and no API shows
 * it: the same three private streams ran S2 at 24.5 us per request or at 40-86 us
 * (one stream: 28.6) with nothing changed but the number of streams the process
 * had created before (profiles/r04_private_streams_queue_mapping.txt).  The first
 * request of every caller stream that would take a private stream therefore runs
 * a short synthetic probe of the request pattern behind that stream (kernels that
 * only wait; the host blocks for ~8 ms and args->stream drains once).  While no
 * live plan relies on the present mapping, other mappings are tried — the private
 * streams are re-created with the next priority (normal, low, high) and behind up to six
 * spacer streams, ~8 ms each — within a WALL-TIME budget (a request: 120 ms,
 * FCP_PRIVATE_VERIFY_BUDGET_MS; fcp_plan_verify_private_streams: its argument).
 * A caller behind which no mapping overlaps keeps
 * its requests on its own stream: the mode then costs nothing instead of a
 * multiple.  (A verdict is kept per stream HANDLE for the life of the plan: a
 * process that destroys and re-creates its streams calls this function again.)
 * FCP_PRIVATE_NO_VERIFY skips all of it (the streams are used as
 * created); FCP_DIAG=private_verify_verbose prints the search.
 * Callers with a warm-up request (every deployment of the reference has one,
 * docs/build_from_source.md:42) call fcp_plan_verify_private_streams there: no
 * serving request then ever pays for the search.
 *
 * Supervision.  A verdict is learnt once, from a synthetic probe; what the private
 * streams buy the caller's REAL traffic — its readers, its host threads, its pace —
 * and whether the mapping still overlaps later, is measured while serving: an
 * online A/B.  An evaluation runs 48 consecutive requests of the caller on
 * args->stream between two timing events there, then 48 on the private streams
 * between two timing events on one of them, and compares the time per byte of
 * work (private / stream order: streams that overlap measure 0.64-0.92; readers
 * right behind their requests 1.13-1.64; sparse traffic ~1.0 — nothing to overlap;
 * a mapping that stopped overlapping 1.1 and more:
 * profiles/r05_caller_threads_grid.txt).  Two consecutive evaluations above 0.97
 * DEMOTE the caller: verdict 0 (a line on stderr only under FCP_DIAG=lane_log), its requests stay on
 * args->stream; two consecutive ones below it re-admit a demoted caller (a trickle
 * at start-up, load later).  Evaluations run at the caller's first eligible
 * request, 256 requests later, then at doubling gaps up to 8192 requests: < 1 %
 * of the traffic runs in the mode that loses.  Results are unaffected at every
 * point.  FCP_LANE_SUPERVISE=0 turns the supervisor off; FCP_LANE_SUPERVISE_PERIOD
 * (largest gap), FCP_LANE_KEEP_RATIO tune it; fcp_plan_private_streams_stats reads
 * it; fcp_plan_verify_private_streams (a new search) starts it over. */
enum { FCP_PRIVATE_NO_CALLER_WAIT = 1u << 0, FCP_PRIVATE_ALWAYS = 1u << 1, FCP_PRIVATE_NO_VERIFY = 1u << 2 };
/* experimental */ int fcp_plan_set_private_streams(fcp_plan_t *plan, int32_t n_streams, uint32_t flags);

/* Diagnostic: do the plan's private streams overlap behind THIS caller stream, in THIS process?  Whether event-linked
 * streams overlap depends on which hardware queues the HIP runtime mapped them to — the creation order of every stream of
 * the process, GPU_MAX_HW_QUEUES, stream priorities — and cannot be told from the API: the same three private streams
 * measured 24.5 us per S2 request or 40-85 us (one stream: 28.6) with nothing changed but the number of streams the
 * process had created before (profiles/r04_private_streams_queue_mapping.txt).  The probe replays the request pattern
 * with kernels that only wait: `requests` kernels of `spin_us` microseconds on grid_blocks x 256 threads, each followed
 * — n_streams - 1 requests later — by its consumer (a stream wait + a one-thread kernel) on `stream`; once back to back
 * on `stream` (*serial_us), once through the private streams (*lanes_us, 0 without private streams); host clock, each
 * ending with a synchronisation of `stream`.  *lanes_us well below *serial_us: they overlap.  (The library runs this
 * probe itself on the first request of every caller stream, see Verification above; the entry point is for harnesses
 * and for processes that pass FCP_PRIVATE_NO_VERIFY.) */
/* experimental */ int fcp_plan_probe_private_streams(fcp_plan_t *plan, void *stream, int32_t requests, int32_t spin_us, int32_t grid_blocks,
                                   double *serial_us, double *lanes_us);
/* What the verification decided for `stream`: *verdict = 1 (its requests take the private streams), 0 (they stay on
 * `stream`: nothing overlapped behind it) or -1 (no request of that stream verified yet, or the mode is off). */
/* experimental */ int fcp_plan_private_streams_verdict(fcp_plan_t *plan, void *stream, int32_t *verdict);
/* The verification at a time of the caller's choosing (warm-up): probes the private streams behind `stream` now and, while
 * no live plan relies on the present mapping, searches another one for at most about budget_ms of wall time (<= 0: 400 ms;
 * one mapping costs ~8 ms, the whole search space ~22 of them).  A negative verdict of an earlier, cheaper look — or a
 * demotion by the supervisor — is forgotten and the search runs again (the supervisor then starts over with an evaluation at
 * the next request); a positive one is returned as it is.  Blocks the
 * host, drains `stream`.  *verdict (optional) as fcp_plan_private_streams_verdict; -1 when the mode is off, or when the
 * plan's requests so far are below the work threshold (they stay on `stream` anyway: nothing is probed).  Call it after
 * the first (warm-up) request of the plan, as the shim does. */
/* experimental */ int fcp_plan_verify_private_streams(fcp_plan_t *plan, void *stream, int32_t budget_ms, int32_t *verdict);
/* What the run-time supervisor of the plan's private streams has seen (see Supervision above). */
typedef struct fcp_private_streams_stats {
  void *supervised_stream;        /* the caller stream under supervision (the first that took the private streams), or NULL   */
  int64_t requests;               /* its requests that were eligible for a private stream so far                              */
  int64_t lane_requests;          /* ... of which ran on one                                                                  */
  int64_t evaluations;            /* completed A/B evaluations (48 requests in stream order, 48 on the private streams)       */
  double stream_order_us_per_mib; /* last evaluation: stream-order time per MiB of work (rows gathered + output written)      */
  double last_ratio;              /* last evaluation: time per byte on the private streams / in stream order                  */
  double worst_ratio;             /* the largest such ratio so far                                                            */
  double keep_ratio;              /* private streams are kept while the ratio stays at or below this (0.97)                   */
  int32_t demoted;                /* 1: the supervisor keeps this caller's requests on its own stream at present              */
  int32_t evaluation_in_progress; /* 1: an evaluation is running or waiting for its timing events                             */
} fcp_private_streams_stats_t;
/* experimental */ int fcp_plan_private_streams_stats(fcp_plan_t *plan, fcp_private_streams_stats_t *out);

/* The cheap half of the same idea, for callers that OWN their buffers: FCP_ORDER_INPUTS_READY is the caller's promise, for
 * every request of the plan, that when fcp_process_feature_columns is CALLED the blob is complete in device memory and
 * nothing still queued or running on args->stream touches the memory malloc_buff returns.  The fused kernel is then
 * launched without the queue's barrier bit, so the command processor need not wait for the queue to drain before it takes
 * the next packet: the BOUNDARY between two requests shrinks — on ONE stream, without events or extra streams (S2 back to
 * back: 28.3 -> 26.0-26.5 us per request, 0.60-0.61 of 8 TB/s; Zipf ids 25.4 -> 23.4).  What it does NOT do on this runtime
 * (round 5, scripts/probes/any_order_probe.hip): start the kernel while blocks of its predecessor still run — behind a
 * kernel whose blocks retire between 10 and 20 us the first block of the next one starts at 21.4 us without the barrier bit,
 * 22.7 us with it, wave slots free from 10 us on — so there is no overlap of a front with a predecessor's tail, only a
 * cheaper hand-over.  Everything queued BEHIND the kernel on args->stream (the consumer) still waits for it, as any
 * stream-ordered command waits for all commands before it — which is also why the gain is only there while requests
 * follow each other directly: an ordinary command between two requests (a consumer kernel, an event record) orders
 * the second request behind the first again; private streams (above) are the tool for that pattern.  NOT for
 * TensorFlow's allocator, which hands out memory that earlier, still queued kernels of the compute stream may be using.
 * Requests that queue work of their own in front of the kernel keep stream order for the kernel; of that work the
 * segment-offset pre-pass is itself launched without the barrier bit (it reads the blob and writes the new arena only:
 * RAGGED as delivered 34.4 -> 33.5 us), the inverse-map memset and the descriptor upload kernel are not.
 * Default: FCP_ORDER_STREAM. */
enum { FCP_ORDER_STREAM = 0, FCP_ORDER_INPUTS_READY = 1 };
/* experimental */ int fcp_plan_set_request_order(fcp_plan_t *plan, int32_t order);
/* experimental */ int fcp_result_wait(const void *buffer, void *stream);
/* A host reader: returns once the request has completed on the device.  What that guarantees is device-scope: copies and
 * kernels issued afterwards (hipMemcpy*, any stream) see the result.  A host that reads the arena DIRECTLY — host-mapped or
 * fine-grained memory — gets no system-scope visibility from it (the completion events carry no system fence, which is what
 * keeps them off the GPU's critical path): such a reader copies through the device or synchronises a stream of its own. */
/* experimental */ int fcp_result_synchronize(const void *buffer);

/* ---- ConcatOutputs (concat_outputs_op_gpu.cu.cc:85-140) ------------------ */
/* out[p, off_k : off_k + dims[k]] = inputs[k][p*dims[k] ...] for k < n.
 * `inputs` is a HOST array of device pointers; the pointer table is passed to
 * the kernel without a separate H2D copy when n is small.  elem_size 4 only
 * (reference registers float and int, :250-251). */
int fcp_concat_outputs(const void *const *inputs, const int32_t *dims,
                       int32_t n, int64_t prefix_size, void *out, void *stream);

/* The same with explicit destinations: input k ([prefix, dims[k]], contiguous, device)
 * goes to columns [col_offsets[k], col_offsets[k] + dims[k]) of the row-major
 * matrix `out` [prefix, out_width].  (ScatterBlock<EmbedDim, Offset>,
 * concat_outputs_op_gpu.cu.cc:85-99, with run-time offsets.) */
int fcp_concat_outputs_scatter(const void *const *inputs, const int32_t *dims,
                               const int32_t *col_offsets, int32_t n,
                               int64_t prefix_size, int32_t out_width, void *out,
                               void *stream);
/* The same for inputs that are column ranges of wider matrices: input k has row stride in_strides[k] floats
 * (>= dims[k]; NULL: contiguous).  The mixed-placement step assembles its output this way from the row-sharded
 * part and every rank's whole-column block. */
int fcp_concat_outputs_scatter_strided(const void *const *inputs, const int32_t *dims,
                                       const int32_t *in_strides, const int32_t *col_offsets,
                                       int32_t n, int64_t prefix_size, int32_t out_width,
                                       void *out, void *stream);
/* Addons>ConcatOutputs `host_inputs` (concat_outputs_op_gpu.cu.cc:186-216): the n
 * HOST tensors ([prefix, dims[k]], 4-byte elements) are packed into one pinned
 * staging buffer (library-owned, per device) and scattered into columns
 * [col_offsets[k], +dims[k]) of `out` [prefix, out_width] by one kernel on `stream`
 * — reading the pinned buffer through its device mapping when the payload is at
 * most 1 MiB (no copy at all), otherwise after ONE asynchronous H2D copy into
 * scratch obtained from `malloc_temp` (the reference's allocate_temp, :189-193;
 * called only then: it may be NULL for payloads of at most 1 MiB).  Calls from
 * several threads overlap: the per-device ring lock covers slot bookkeeping only.
 * With FCP_LAYOUT_CONCAT `out` is the group's
 * matrix inside the FeatureColumnProcess arena, whose FCP_FORM_EXTERNAL slots are
 * exactly these columns.  No stream synchronisation (the reference blocks, :234);
 * the host tensors may be reused when the call returns. */
int fcp_concat_outputs_host(const void *const *host_inputs, const int32_t *dims,
                            const int32_t *col_offsets, int32_t n,
                            int64_t prefix_size, int32_t out_width, void *out,
                            fcp_alloc_fn malloc_temp, void *malloc_temp_ctx,
                            int32_t device, void *stream);

/* ---- request staging: ConcatInputs + the H2D copy as one step -- */
/* The reference packs N host tensors with N mempcpy calls on one CPU thread into a
 * pageable TF tensor (concat_inputs_ops.cc:69-76) which TF then copies H2D.  A
 * stager owns a ring of pinned host buffers with device twins: fcp_stager_stage
 * packs the tensors (same bytes, offsets and shapes as fcp_concat_inputs) with
 * `n_threads` worker threads straight into pinned memory and enqueues ONE
 * hipMemcpyAsync on the stager's own copy stream (so the copy of request k+1
 * overlaps the kernel of request k); `stream` is made to wait for that copy.  The
 * returned pointers stay valid until the slot is reused, i.e. for the next depth-1
 * calls; the work that reads them must be enqueued on `stream` before the next call.
 * (A plan with private streams runs that work elsewhere: fcp_process_feature_columns
 * then files the blob it was given next to the arena, and the stager waits for that
 * reader — the copy stream, or the host for a zero-copy slot — before it overwrites
 * the slot.  Nothing to do for the caller.)
 *
 * fcp_stager_stage_narrow additionally converts the int64 inputs flagged in
 * `narrow_int64[n_inputs]` to int32 while packing (values outside [0, 2^31) become
 * -1, an invalid id / row either way): half the PCIe bytes for id and index tensors.
 * The plan consuming such a blob declares those inputs as 4-byte (FCP_IDS_I32 /
 * FCP_SEG_IDS_I32); results are unchanged.
 *
 * FCP_STAGER_ZERO_COPY (fcp_stager_create_ex): no copy at all — the ring is pinned
 * memory mapped into the device's address space and the returned "device blob" is
 * that mapping: the kernels fetch the ids over PCIe themselves.  Fewer runtime calls
 * per request and no copy engine in the path (S2: 65 us per request steadily, where
 * the copying form swings between 63 and 150 us with the host's load; lone-request
 * latency 100-117 vs 121-137 us), at the price of a kernel that holds its CUs for the
 * duration of the transfer.  A slot is repacked only after the work that read it has
 * finished (the call waits on the host if it must).
 *
 * (r5) Inside one request the pack and the copy overlap: the inputs are packed in up to four groups (FCP_STAGER_GROUPS) and
 * every group is shipped the moment its last byte is in the pinned buffer (by the calling thread, which watches the pack
 * workers instead of packing) — a lone request costs pack + copy / 4 + kernel instead of pack + copy + kernel.
 * (Groups are used when the caller is not issuing back to back — more than 40 us since the previous call returned: under
 * load they cost throughput, S2 58 -> 66 us per request, because the caller no longer packs.)
 * The copies themselves are KERNELS on the stager's copy stream that read the pinned ring through its device mapping
 * (FCP_STAGER_COPY_KERNEL, the default since round 5): hipMemcpyAsync's SDMA submission blocks its caller for 6-14 ms a few
 * times per thousand calls on the boxes this was measured on (profiles/r05_pcie_staging_stalls.txt), kernel copies never
 * did.  FCP_STAGER_COPY_SDMA asks for the copy engine; FCP_STAGER_COPY=kernel|sdma overrides both at run time. */
typedef struct fcp_stager fcp_stager_t;
enum { FCP_STAGER_DEFAULT = 0, FCP_STAGER_ZERO_COPY = 1, FCP_STAGER_COPY_KERNEL = 2, FCP_STAGER_COPY_SDMA = 4 };
int fcp_stager_create(int32_t device, int64_t capacity_bytes, int32_t max_inputs,
                      int32_t max_rank_sum, int32_t depth, int32_t n_threads,
                      fcp_stager_t **stager);
int fcp_stager_create_ex(int32_t device, int64_t capacity_bytes, int32_t max_inputs,
                         int32_t max_rank_sum, int32_t depth, int32_t n_threads,
                         uint32_t flags, fcp_stager_t **stager);
int fcp_stager_stage(fcp_stager_t *stager, const fcp_host_tensor_t *inputs,
                     int32_t n_inputs, void *stream, const void **device_blob,
                     int64_t *blob_bytes, const int32_t **offsets,
                     const int32_t **shapes);
int fcp_stager_stage_narrow(fcp_stager_t *stager, const fcp_host_tensor_t *inputs,
                            int32_t n_inputs, const uint8_t *narrow_int64, void *stream,
                            const void **device_blob, int64_t *blob_bytes,
                            const int32_t **offsets, const int32_t **shapes);
/* The general form: modes[n_inputs] (NULL: all FCP_STAGE_COPY) says what happens to each input while it is packed.
 * FCP_STAGE_SEG_TO_CSR turns the sorted row ids of a multi-hot feature — an int32 / int64 tensor [nnz], or the
 * SparseTensor indices [nnz, k] whose column 0 they are — into the int32 row offsets[rows + 1] the kernels want
 * (mode_args[i] = rows; the plan declares that input FCP_SEG_CSR_I32, rank 1): the host reads those bytes anyway to
 * pack them, the device then needs neither the segment-offset pre-pass nor the in-block search, and 16 bytes per id
 * shrink to 4 bytes per ROW on the wire (RAGGED, BASELINE configs[3]: 15.7 MB of blob -> 3.1 MB with narrowed ids). */
enum { FCP_STAGE_COPY = 0, FCP_STAGE_NARROW_I64 = 1, FCP_STAGE_SEG_TO_CSR = 2 };
int fcp_stager_stage_ex(fcp_stager_t *stager, const fcp_host_tensor_t *inputs, int32_t n_inputs,
                        const uint8_t *modes, const int64_t *mode_args, void *stream,
                        const void **device_blob, int64_t *blob_bytes, const int32_t **offsets,
                        const int32_t **shapes);
int fcp_stager_destroy(fcp_stager_t *stager);
/* What the stager has seen so far: staging calls, copy calls (one per group), how long the slowest copy CALL held its host
 * thread, how many held it for more than a millisecond (the "14 ms stalls" of profiles/r04_pcie_staging_memcpy_anomaly.txt),
 * requests the zero-copy fallback served. */
typedef struct fcp_stager_stats {
  int64_t calls, copy_calls, copy_calls_over_1ms, fallback_switches, requests_with_blocked_copy;
  double max_copy_call_us;
} fcp_stager_stats_t;
int fcp_stager_stats(fcp_stager_t *stager, fcp_stager_stats_t *out);

/* ---- Addons>ConcatInputs in its staged form (host only; replaces concat_inputs_ops.cc:42-77) ---- */
/* The same packing as fcp_stager_stage_ex — modes[n_inputs] / mode_args[n_inputs] as there, NULL = plain
 * fcp_concat_inputs — into a caller-owned blob, on the calling thread, without a stager or a device: what the TF
 * shim's ConcatInputsOp runs (its output 0 is the blob; TensorFlow copies it to the GPU).  The reference's op copies
 * every input byte for byte (RAGGED, BASELINE configs[3]: 15.7 MB per request); with the modes of the plan file's
 * stage section the blob carries int32 ids and int32 row offsets (3.1 MB) and the device runs neither the
 * segment-offset pre-pass nor the in-block search.  The consuming plan is the STAGED plan (PlanSpec.staged()):
 * narrowed inputs declared 4-byte, converted ones FCP_SEG_CSR_I32 of rank 1. */
int fcp_concat_inputs_ex_sizes(const fcp_host_tensor_t *inputs, int32_t n_inputs,
                               const uint8_t *modes, const int64_t *mode_args,
                               int64_t *blob_bytes, int32_t *rank_sum);
int fcp_concat_inputs_ex(const fcp_host_tensor_t *inputs, int32_t n_inputs,
                         const uint8_t *modes, const int64_t *mode_args, void *blob,
                         int64_t blob_capacity, int32_t *offsets, int32_t *shapes);
/* The same on a worker pool: the reference's op packs on one thread (concat_inputs_ops.cc:42-77), which for RAGGED is
 * 1.4 ms per request of the staged pack (0.5 ms of plain copying) — longer than everything the GPU does with it.  A
 * pool is a set of sleeping threads that split one call's inputs into ranges of about equal INPUT bytes; the calling
 * thread works too.  One call at a time uses a pool: a second concurrent caller packs on its own thread instead of
 * waiting (so an op instance shared by several serve workers never blocks on it).  Host only. */
typedef struct fcp_pack_pool fcp_pack_pool_t;
int fcp_pack_pool_create(int32_t n_threads, fcp_pack_pool_t **pool);
int fcp_pack_pool_destroy(fcp_pack_pool_t *pool);
int fcp_concat_inputs_ex_pool(fcp_pack_pool_t *pool /* NULL: this thread only */,
                              const fcp_host_tensor_t *inputs, int32_t n_inputs,
                              const uint8_t *modes, const int64_t *mode_args,
                              void *blob, int64_t blob_capacity, int32_t *offsets, int32_t *shapes);
/* The stage section of a column-plan file (version 3, written by `python -m recom_amd.graph --staged`):
 *   stage N symbols_input K / N lines "mode rows_symbol"
 * N = number of Addons>ConcatInputs inputs of the rewritten graph (= the plan's host inputs); modes[i] = FCP_STAGE_*
 * of input i; rows_symbol[i] = for FCP_STAGE_SEG_TO_CSR inputs the index into the `symbols` vector of the row count
 * (mode_args[i] = symbols[rows_symbol[i]]), else -1; *symbols_input = which ConcatInputs input IS that symbols
 * vector (int32[n_symbols]; the rewritten graph wires it in as the op's last input), or -1 when nothing is
 * converted.  *n_inputs = 0: the file has no stage section (a plain plan).  Up to `capacity` entries are written. */
int fcp_plan_file_stage_info(const char *path, int32_t *n_inputs, uint8_t *modes,
                             int32_t *rows_symbol, int32_t capacity, int32_t *symbols_input);

/* ---- plan builder from a GraphDef (replaces CudaEmitter::Optimize, cuda_emitter.cc:80-116) ---- */
/* The non-codegen half of the reference's CudaEmitter as ONE in-process call for the retained Grappler pass: where
 * the reference generates CUDA text per feature column (EmitFCCode, cuda_emitter.cc:975-1178), runs nvcc, caches the
 * .so by md5 and rewrites the graph (Rewrite, :2496-2656), the pass serialises its GraphDef, calls fcp_graph_build and
 * parses what comes back.  `graphdef`: a serialized tensorflow.GraphDef in the form the reference's emitter sees (after
 * the lookup optimizers, lookup_optimizer.cc:157-440).  The column plan is WRITTEN to `plan_path` (the file the
 * rewritten FeatureColumnProcess names in `dlpath`); *rewritten receives the serialized rewritten GraphDef
 * (malloc'd; fcp_graph_free) unless `rewritten` is NULL; *description a human-readable summary (fcp_graph_free), may
 * be NULL.  FCP_ERR_UNSUPPORTED: no ConcatV2 of embedding lookups in this graph ("nothing to fuse": the pass leaves
 * the graph alone).  No TensorFlow, no protobuf library, no Python, no device.  The same walk exists as an offline
 * tool (`python -m recom_amd.graph`); both write identical plan files (tests/test_graph_plan.py). */
enum {
  FCP_GRAPH_HOST_CONCAT_EXTERNAL = 1u << 0, /* non-lookup concat inputs stay Addons>ConcatOutputs host inputs (the
                                               reference's wiring) instead of passthrough columns                 */
  FCP_GRAPH_STAGED = 1u << 1,               /* the staged plan + stage section; ConcatInputs gets `_fcp_plan`       */
  FCP_GRAPH_NO_PRUNE = 1u << 2              /* keep the replaced subgraphs in the output graph                     */
};
int fcp_graph_build(const void *graphdef, size_t n_bytes, uint32_t flags, const char *plan_path,
                    void **rewritten, size_t *rewritten_bytes, char **description);
void fcp_graph_free(void *p);

/* ---- multi-GPU exchange (no reference counterpart) ---------- */
/* The ONE collective of the sharded path: an all-to-all partitioned along the batch,
 * issued as grouped ncclSend / ncclRecv (RCCL) to every peer at once so that all
 * xGMI links of the GPU carry traffic concurrently, on the request's stream, between
 * the partial kernel and fcp_shard_finalize / fcp_concat_outputs.  RCCL is bound at
 * run time (librccl.so.1); FCP_ERR_UNSUPPORTED where it is missing.
 *
 * A communicator belongs to one GPU of one process (one process per GPU).  Rank 0
 * calls fcp_comm_unique_id and ships the 128 bytes to the other ranks by any
 * host-side channel; every rank then calls fcp_comm_create (collective). */
#define FCP_COMM_ID_BYTES 128
#define FCP_MAX_GROUPS_ABI 16 /* fcp_plan_desc_t::n_groups is at most this */
typedef struct fcp_comm fcp_comm_t;
int fcp_comm_unique_id(uint8_t *id /* [FCP_COMM_ID_BYTES] */);
int fcp_comm_create(const uint8_t *id, int32_t rank, int32_t world, int32_t device,
                    fcp_comm_t **comm);
int fcp_comm_destroy(fcp_comm_t *comm);
int fcp_comm_rank(const fcp_comm_t *comm, int32_t *rank, int32_t *world);
/* The batch split every exchange uses: contiguous, the first rows % world ranks get
 * one row more. */
int fcp_shard_batch_slice(int64_t rows, int32_t world, int32_t rank, int64_t *begin,
                          int64_t *count);
/* Row sharding: `partial` = this rank's [rows, width] partial sums (a row-sharded
 * plan's group matrix); on return (enqueued) `slices` holds [world, row_count, width]:
 * rows [row_begin, row_begin + row_count) of every rank's partial, in rank order —
 * the input of fcp_shard_finalize. */
int fcp_shard_exchange(fcp_comm_t *comm, const void *partial, int64_t rows,
                       int64_t width, void *slices, int64_t *row_begin,
                       int64_t *row_count, void *stream);
/* Column sharding: `block` = this rank's [rows, widths[rank]] final column block;
 * `recv` receives, back to back, the [row_count, widths[g]] blocks of g = 0..world-1
 * (fcp_concat_outputs[_scatter] puts them side by side). */
int fcp_shard_exchange_columns(fcp_comm_t *comm, const void *block, int64_t rows,
                               const int32_t *widths, void *recv, int64_t *row_begin,
                               int64_t *row_count, void *stream);
/* One native call per sharded request: partial kernel -> exchange -> finalize (row
 * mode, FCP_PLACE_ROW_SHARD) or concat (FCP_PLACE_COLUMN_SHARD) of concat group
 * `group`, all enqueued on args->stream, from buffers the object owns (a ring of 3;
 * args' allocator callbacks are ignored).  max_rows / max_arena_bytes bound the
 * requests it will see (fcp_plan_arena_bytes); col_widths[world]: column mode only.
 * *out: device [row_count, width] of this rank's batch slice, valid for the next two
 * calls.  Calls may come on different streams and host threads: they are serialised on
 * the step object for the duration of the ENQUEUE (a ring entry waits for its previous
 * use; RCCL wants its collectives issued one at a time and in the same order on every
 * rank), the enqueued work of different streams still overlaps on the GPU. */
typedef struct fcp_shard_step fcp_shard_step_t;
int fcp_shard_step_create(fcp_plan_t *plan, fcp_comm_t *comm, int32_t mode,
                          int32_t group, int64_t max_rows, int64_t max_arena_bytes,
                          const int32_t *col_widths, fcp_shard_step_t **step);
int fcp_shard_step_run(fcp_shard_step_t *step, const fcp_process_args_t *args,
                       void **out, int64_t *row_begin, int64_t *row_count);
int fcp_shard_step_destroy(fcp_shard_step_t *step);

/* ---- multi-GPU finalize (no reference counterpart) --------- */
/* After the all-to-all of per-rank partial sums: out = sum over `world`
 * slices in rank order; for MEAN columns divide by the segment length read
 * from the same blob.  partial_slices: device [world, rows, width]. */
int fcp_shard_finalize(fcp_plan_t *plan, const fcp_process_args_t *args,
                       int32_t group, const void *partial_slices,
                       int32_t world, int64_t row_begin, int64_t row_count,
                       void *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FCP_HIP_H_ */
