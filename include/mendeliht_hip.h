/*
 * mendeliht_hip.h -- C ABI of the MI355X-native IHT hot path.
 *
 * Drop-in boundary for MendelIHT.jl's IHT inner loop.  The reference has no
 * FFI layer; its seam is Julia dispatch on the design-matrix type
 * (`fit_iht(y, x::AbstractMatrix{T}, z)` src/fit.jl:60-63,
 *  `cv_iht` src/cross_validation.jl:60-63, `IHTVariable{T,M}`
 *  src/data_structures.jl:4).  Each entry point below names the reference
 * method(s) it replaces; INTEGRATION.md shows the `ccall` glue a maintainer
 * adds on the Julia side (julia/MendelIHTHip.jl).
 *
 * Conventions: every function returns an `int` status (MIH_OK = 0); all
 * pointers are HOST pointers unless the name says `_dev`; matrices are
 * column-major (Julia layout); indices crossing the boundary are 0-based
 * unless stated; the library owns device memory behind opaque handles and the
 * caller owns every host buffer.  A handle is immutable after creation and may
 * be shared by host threads; each fit call builds its own workspace + stream.
 */
#ifndef MENDELIHT_HIP_H
#define MENDELIHT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes <-> Julia exceptions (src/fit.jl:87-101,259-260;
 * src/data_structures.jl:63-85; src/utilities.jl:554,975-993) */
enum {
    MIH_OK = 0,
    MIH_BAD_DIM = 1,        /* DimensionMismatch */
    MIH_BAD_ARG = 2,        /* ArgumentError / DomainError / AssertionError */
    MIH_NOT_CENTERED = 3,   /* "x is not centered!" fit.jl:98 */
    MIH_NAN_LOGL = 4,       /* "Loglikelihood function is NaN" fit.jl:259 */
    MIH_INF_LOGL = 5,       /* "Loglikelihood function is Inf" fit.jl:260 */
    MIH_HIP_ERROR = 6,
    MIH_OOM = 7,
    MIH_NO_DEVICE = 8
};

/* Distributions / links of the GLM (GLM.jl, Distributions.jl; fit.jl:66-67) */
enum { MIH_NORMAL = 0, MIH_BERNOULLI = 1, MIH_POISSON = 2, MIH_NEGBIN = 3,
       MIH_GAMMA = 4, MIH_INVGAUSS = 5 };   /* the distributions loglik_obs covers (src/utilities.jl:32-43) */
enum { MIH_IDENTITY = 0, MIH_LOGIT = 1, MIH_LOG = 2, MIH_PROBIT = 3, MIH_CLOGLOG = 4, MIH_CAUCHIT = 5,
       MIH_INVERSE = 6, MIH_INVSQUARE = 7, MIH_SQRT = 8 };   /* GLM.jl Link types accepted as `l` */
enum { MIH_ESTR_NONE = 0, MIH_ESTR_MM = 1, MIH_ESTR_NEWTON = 2 };

typedef struct mih_mat mih_mat;     /* device-resident design matrix */

/* ---- library / device ------------------------------------------------------ */
int mih_device_count(int *count);
/* thread-local message of the last failing call on this host thread */
int mih_last_error(char *buf, size_t len);
int mih_version(int *major, int *minor);     /* 0.7: VCF text streamed into a dosage matrix (mih_vcf_*, mih_dosage_create_vcf), and hard calls packed into the 2-bit matrix on the device (mih_snp_builder_*, mih_snp_create_dosage, mih_snp_create_vcf), and counts and subsets of the 2-bit matrix (mih_snp_counts, mih_snp_subset), and the kinship matrix and related-pair screen (mih_grm, mih_grm_pairs), and its leading eigenpairs (mih_grm_eig), and the SNP correlation band and LD pruning (mih_ld_band, mih_ld_pairs, mih_ld_prune): additions, the version stays; 0.6: BGEN streamed into a dosage matrix (mih_dosage_create_bgen, mih_dosage_regrid); 0.5: the 16-bit dosage matrix (mih_dosage_*); 0.4: cv_threads, mih_cv_allgather, column-sharded lock-step drivers */
/* sizeof(mih_fit_params), sizeof(mih_fit_result), sizeof(mih_mv_result), sizeof(mih_comm): lets a binding
 * check its struct mirrors against the library it loaded. */
int mih_abi_sizes(int64_t *sizes, int32_t n);

/* ---- design matrix: replaces SnpArrays.SnpLinAlg{T}(::SnpArray; model=ADDITIVE_MODEL,
 *      center, scale, impute) as constructed at src/wrapper.jl:68-69 and test/L0_reg_test.jl:11.
 * bed_cols: p columns of PLINK .bed body (after the 3-byte header), each
 * col_stride_bytes >= ceil(n/4) bytes, codes 00->0, 01->missing, 10->1, 11->2.
 * dtype is the caller's element type T, 64 or 32 (src/MendelIHT.jl:39: Float = Union{Float64, Float32}; MIH_BAD_ARG otherwise).  It
 * changes nothing on the device -- the 2-bit matrix has no element type there and every dot product is exact fixed point
 * recombined in Float64 -- so a SnpLinAlg{Float32} caller gets results at least as accurate as the reference's all-Float32 run:
 * the binding converts y, z to Float64 on the way in and the model to Float32 on the way out.  Uploads once; computes mu_j (mean of non-missing
 * dosages) and sinv_j = 1/sqrt(mu_j(1-mu_j/2)) (1 when that sqrt is 0) on device. */
int mih_snp_create(const uint8_t *bed_cols, int64_t n, int64_t p, int64_t col_stride_bytes,
                   int center, int scale, int impute, int dtype, int device, mih_mat **out);
/* On-device synthetic SnpArray for benchmarks: maf_j ~ U(0,0.5), g_ij ~ Binomial(2, maf_j),
 * each entry missing with probability missing_rate (distributions of
 * src/simulate_utilities.jl:33-47,85-101; counter-based hash RNG, seed-reproducible). */
int mih_snp_create_synthetic(int64_t n, int64_t p, uint64_t seed, double missing_rate,
                             int center, int scale, int impute, int device, mih_mat **out);
/* Columns [col_offset, col_offset + p) of the same synthetic matrix (the generator is keyed by
 * (seed, global column)): one shard of a column-sharded fit. */
int mih_snp_create_synthetic_shard(int64_t n, int64_t p, int64_t col_offset, uint64_t seed,
                                   double missing_rate, int center, int scale, int impute,
                                   int device, mih_mat **out);
/* Dense Float64 design matrix (the reference's `x::Matrix{Float64}` path), n x p column-major. */
int mih_dense_create(const double *x, int64_t n, int64_t p, int device, mih_mat **out);
/* `x::Matrix{Float32}` (test/L0_reg_test.jl:245, test/cv_iht_test.jl:41): the matrix is STORED in Float32 (half
 * the HBM traffic of X'r); y, the model and every sum stay Float64, so results are at least as accurate as the
 * reference's all-Float32 run. */
int mih_dense_create_f32(const float *x, int64_t n, int64_t p, int device, mih_mat **out);
int mih_dense_create_synthetic(int64_t n, int64_t p, uint64_t seed, int device, mih_mat **out);
/* Genotype dosages (VCF DS / GT, BGEN) on the grid d = num / denom in [0, 2], stored as 16-bit numerators: 4x less HBM
 * than the reference's dense Matrix{Float64} of the same values.  num is n x p column-major with column stride col_stride
 * (>= n); 1 <= denom <= 32767; 0xFFFF marks a missing entry, any other num > 2 denom is MIH_BAD_ARG.  The handle is a dense
 * matrix to every fit and holds the STANDARDIZED genotypes of standardize_genotypes! (src/wrapper.jl:406-423), as
 * SnpLinAlg(center, scale, impute) does: mu_j = mean of the non-missing d, sigma_j = sqrt(mu_j (1 - mu_j / 2)),
 * x_ij = (d_ij - mu_j) / sigma_j (d_ij - mu_j where sigma_j = 0), 0 where missing (imputed by the mean); an all-missing
 * column is all zeros.  (The reference's own function throws on a missing entry: wrapper.jl:411 reads an undefined `t`.) */
int mih_dosage_create(const uint16_t *num, int64_t n, int64_t p, int64_t col_stride, int32_t denom, int device, mih_mat **out);
/* A seeded synthetic dosage matrix generated on the device (no host upload): hard calls Binomial(2, rho_j),
 * rho_j ~ U(0, 0.5), moved by up to +-0.1 on the grid of denom and clamped to [0, 2]; each entry missing with
 * probability missing_rate. */
int mih_dosage_create_synthetic(int64_t n, int64_t p, uint64_t seed, int32_t denom, double missing_rate, int device, mih_mat **out);
/* A dosage handle built straight from a BGEN v1.2 file: the n x ncols matrix of the genotype blocks whose 4-byte length fields
 * sit at the file offsets block_offset[0 .. ncols) (increasing), as the caller's walk of the variant headers found them:
 * consecutive variants are read in runs of a few MB, offsets that skip variants block by block (no skipped block is read).
 * Accepted: layout 2, compression 0 (none) or 1 (zlib), unphased, every sample diploid, the same B in 1..16 bits per
 * probability in every block.  Dosage d = (2 k_BB + k_AB) / (2^B - 1) (the ALT allele counted), 0xFFFF where the ploidy byte
 * marks the sample missing; the result is on the matrix's own reduced grid -- numerators and *denom_out as
 * genotypes.genotype_values gives them for these columns.  threads = 0: the library's default (at most 8 workers).
 * On a block that is refused or cannot stream: MIH_BAD_ARG, nothing allocated, *bad_block the first such block in file order
 * (0-based among the ncols) and *bad_what why (MIH_BGEN_*).  Codes 1-6 are read_bgen's refusals, by its order within a block;
 * 10-13 mark a file that does not fit this path (a reader falls back to its general one there). */
enum {
    MIH_BGEN_CORRUPT = 1,       /* the inflated length is not the stored one */
    MIH_BGEN_HEADER = 2,        /* N or K of the block disagrees with the file header (K != 2: not biallelic) */
    MIH_BGEN_PLOIDY = 3,        /* pmin, pmax or a sample's ploidy other than 2 */
    MIH_BGEN_PHASED = 4,        /* phased data */
    MIH_BGEN_BITS = 5,          /* B outside 1..32 */
    MIH_BGEN_SUM = 6,           /* a non-missing sample's probabilities sum above 1 */
    MIH_BGEN_DEEP = 10,         /* B above 16 */
    MIH_BGEN_MIXED = 11,        /* B differs from the first block's */
    MIH_BGEN_FINE = 12,         /* 16 bits whose reduced denominator is above 32767 (fractional dosages) */
    MIH_BGEN_MALFORMED = 13     /* a block too short for what it holds, or a zlib stream that does not inflate */
};
int mih_dosage_create_bgen(const char *path, int64_t n, int64_t ncols, const int64_t *block_offset, int compression,
                           int threads, int device, mih_mat **out, int32_t *denom_out, int64_t *bad_block, int32_t *bad_what);
/* A dosage handle built straight from a VCF file, plain text, gzip (one or several members) or BGZF; the GPU tokenises the
 * sample fields.  mih_vcf_open needs no device: it finds the container from the file's bytes (a name ending in .gz must hold
 * gzip, any other name text), scans the inflated text once -- BGZF blocks inflated by `threads` workers (0: the library's
 * default; at most 8 in this pass either way), a gzip stream serially -- for the one #CHROM line (n = its fields - 9), the number of records (lines
 * that do not start with '#') and the longest line, and cuts the text into chunks of whole lines of at most
 * max(chunk_bytes, longest line) bytes (chunk_bytes = 0: 8 MB), the unit pass 2 stages.  mih_dosage_create_vcf streams records
 * [rec0, rec0 + nrec) into an n x nrec matrix: field 0 reads GT (one or two alleles of 0 1 . separated by / or |; the count of
 * 1s over the denominator 1), field 1 reads DS (D+, D+., D+.D*, .D+; at most 4 decimals once trailing zeros are dropped, at most 2,
 * at most 32 bytes) on the grid 10^4 / g, g the gcd of 10^4 and every positive numerator: numerators and *denom_out as
 * genotypes.genotype_values gives them for these records.  The key's place in FORMAT is found per record; a sample field that
 * ends before it, an empty token and '.' are missing (0xFFFF).  mih_vcf_meta: CHROM POS ID REF ALT of the records just read,
 * tab-separated, one line each; mih_vcf_header: the #CHROM line.  Both copy at most len bytes and report the full length in
 * *need.  Whatever is outside this (MIH_VCF_*) is refused with MIH_BAD_ARG, nothing left allocated or open, *bad_record the
 * least 0-based record index found bad and *bad_what why: a reader hands such a file to its general path. */
enum {
    MIH_VCF_RAGGED = 1,         /* a record without exactly 9 + n tab-separated fields (an empty line is one) */
    MIH_VCF_TOKEN = 2,          /* a token outside the grammar; a '\r' or a non-ASCII byte in a record; POS not all digits */
    MIH_VCF_RANGE = 3,          /* a DS value above 2 */
    MIH_VCF_DECIMALS = 4,       /* a fifth significant decimal */
    MIH_VCF_NOKEY = 5,          /* FORMAT does not hold the wanted key */
    MIH_VCF_MULTIALLELIC = 6,   /* a comma in ALT */
    MIH_VCF_HEADER = 7,         /* no #CHROM line before the first record, a second one, a '\r' in a # line, no sample column */
    MIH_VCF_CONTAINER = 8,      /* the bytes are not what the name says; a member that does not inflate or is truncated */
    MIH_VCF_IO = 9,             /* not a regular file that can be opened and read (missing, a directory, a pipe), or one that changed */
    MIH_VCF_NOT_HARD_CALL = 10  /* mih_snp_create_vcf only: a DS value other than 0, 1 or 2 (the 2-bit matrix holds hard calls) */
};
typedef struct mih_vcf mih_vcf;
int mih_vcf_open(const char *path, int threads, int64_t chunk_bytes, mih_vcf **out, int64_t *bad_record, int32_t *bad_what);
int mih_vcf_info(const mih_vcf *v, int64_t *n, int64_t *nrecords, int32_t *container /* 0 text, 1 gzip, 2 BGZF */, int64_t *longest_line);
int mih_vcf_header(const mih_vcf *v, char *buf, int64_t len, int64_t *need);
int mih_dosage_create_vcf(mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads, int device, mih_mat **out,
                          int32_t *denom_out, int64_t *bad_record, int32_t *bad_what);
int mih_vcf_meta(const mih_vcf *v, char *buf, int64_t len, int64_t *need);
/* The host work of mih_dosage_create_vcf alone, for measurements: the same workers read and inflate every chunk of the file
 * into ordinary memory and drop it -- no device, no look at the text.  *bytes: the inflated bytes. */
int mih_vcf_inflate(const mih_vcf *v, int threads, int64_t *bytes);
int mih_vcf_close(mih_vcf *v);
/* Hard calls in a dosage handle -- every numerator 0, denom, 2 denom or 0xFFFF, which is what a VCF GT field and a hard-call
 * BGEN file give -- packed on the device into the 2-bit matrix of mih_snp_create: a quarter of a byte per genotype instead of
 * two, and the matrix-core X'r pass, the 19-residual fused pass and the resident IHT step instead of the dense kernels.  The
 * dosage counts ALT alleles as .bed counts allele 2, so the result is, bit for bit, the handle mih_snp_create builds from the
 * .bed codes 0 -> 00, 1 -> 10, 2 -> 11, missing -> 01 of the same genotypes (image, mu, sinv, missing lists; an all-missing
 * column is whatever mih_snp_create makes of it).  center, scale, impute, dtype: as mih_snp_create.
 *
 * A builder takes the matrix panel by panel, so that n x p u16 never has to exist: mih_snp_builder_create allocates the n x p
 * image, mih_snp_builder_add packs a dosage handle of n rows into columns [col0, col0 + dosage.p) -- panels in any order, col0
 * any column (two panels may share a group of 32 columns: a pack writes only the 16-byte lane records of its own columns); the
 * call returns when the panel has been read, and the panel may be destroyed -- and mih_snp_builder_finish, once every column has
 * been added, computes the statistics and the missing lists and hands out an ordinary immutable matrix handle (with the reserve
 * rule of mih_snp_create); the builder is then empty and is still to be destroyed.  mih_snp_builder_destroy releases whatever the
 * builder still owns, at any point.  Refusals: a panel with another row count or columns outside the matrix MIH_BAD_DIM; a column
 * added twice, or a numerator that is no hard call, MIH_BAD_ARG with *bad_col (may be NULL) the least offending 0-based column
 * of the matrix and a message naming it 1-based; finish with columns missing MIH_BAD_ARG.  After a numerator has been refused
 * the builder accepts nothing more and cannot finish.  mih_snp_create_dosage is create + one add + finish. */
typedef struct mih_snp_builder mih_snp_builder;
int mih_snp_builder_create(int64_t n, int64_t p, int center, int scale, int impute, int dtype, int device, mih_snp_builder **out);
int mih_snp_builder_add(mih_snp_builder *b, int64_t col0, const mih_mat *dosage, int64_t *bad_col);
int mih_snp_builder_finish(mih_snp_builder *b, mih_mat **out);
int mih_snp_builder_destroy(mih_snp_builder *b);
int mih_snp_create_dosage(const mih_mat *dosage, int center, int scale, int impute, int dtype, mih_mat **out, int64_t *bad_col);
/* Records [rec0, rec0 + nrec) of an opened VCF file streamed straight into the 2-bit matrix: pass 2 of mih_dosage_create_vcf
 * with the tokeniser pointed at a per-worker u16 panel of the chunk's records and the pack queued behind it on the worker's
 * stream, so device memory holds the 2-bit image and the workers' staging, never n x nrec u16.  field 0: GT; field 1: DS where
 * every value is exactly 0, 1 or 2 (any spelling the DS grammar takes).  A record with another DS value is refused as
 * MIH_VCF_NOT_HARD_CALL; every other refusal, and mih_vcf_meta afterwards, are mih_dosage_create_vcf's. */
int mih_snp_create_vcf(mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads, int center, int scale, int impute, int dtype,
                       int device, mih_mat **out, int64_t *bad_record, int32_t *bad_what);
/* Quality control and sample selection on the device, for 2-bit handles (any other handle: MIH_BAD_ARG) -- what
 * SnpArrays.filter(s; min_success_rate_per_row, min_success_rate_per_col, min_maf) and the selection of samples do before any
 * fit_iht in manuscript/NFBC_sim/NFBC_data_qc.jl and manuscript/UKBB_metabolomic/data_process.jl, and what SnpArrays.maf gives
 * src/utilities.jl:687-693 -- without the matrix leaving the device.
 *
 * mih_snp_counts: the genotype counts of every kept column over the kept rows, and the missing genotypes of every kept row
 * among the kept columns.  row_keep (n bytes) and col_keep (p bytes) are 0 / 1 masks in host memory, NULL = everything;
 * col_counts (4 p, may be NULL) receives n0, n1, n2, nmiss of column j in col_counts[4 j ..], zeros for a column that is not
 * kept; row_missing (n, may be NULL) receives 0 for a row that is not kept.  All integers, so exact.  n1 and n2 are masked
 * population counts in one pass over the tiles, nmiss and row_missing come from the missing lists alone, n0 is the rest:
 * with col_counts == NULL the tiles are not read. */
int mih_snp_counts(const mih_mat *h, const uint8_t *row_keep, const uint8_t *col_keep, int32_t *col_counts, int32_t *row_missing);
/* mih_snp_subset: rows `rows` and columns `cols` of a 2-bit matrix as a new, ordinary, immutable handle on the same device --
 * bit for bit the handle mih_snp_create builds from the .bed codes of the selected genotypes (image, mu and sinv over the kept
 * rows, missing lists), which a `train` mask of a fit is not: mu and sinv of a matrix are taken over all of its rows.  rows
 * (nrows entries) and cols (ncols entries) are strictly increasing 0-based indices in host memory, NULL = all.  The source is
 * only read and stays usable; beyond source and result the device holds O(n + p) bytes, and no genotype crosses the host link.
 * center, scale, impute, dtype and the reserve rule: as mih_snp_create.  Refusals (MIH_BAD_ARG, nothing allocated): a handle
 * that is not 2-bit, an empty selection, an index out of range, indices that are not strictly increasing. */
int mih_snp_subset(const mih_mat *h, const int64_t *rows, int64_t nrows, const int64_t *cols, int64_t ncols,
                   int center, int scale, int impute, int dtype, mih_mat **out);
/* mih_snp_transpose: the 2-bit matrix of the TRANSPOSED genotypes -- SNPs as rows, samples as columns, n_out = p, p_out = n -- as a
 * new, ordinary, immutable handle on the same device, made there (no genotype crosses the host link).  It is bit for bit the handle
 * mih_snp_create builds from the .bed encoding of the transposed code matrix: the tiles with their zero pad rows and columns, mu
 * and 1/sigma (now per SAMPLE, over its observed SNPs), the ascending missing lists and their total.  Everything that takes a 2-bit
 * handle takes it: mih_snp_export_bed, mih_snp_counts, mih_xtv*, a fit.  Its X'r pass is the dense forward product of the source
 * (mih_xb_dense).  The stored tile is a matrix-core operand with the row axis as K, so no image can be contracted over its columns:
 * this second image is the way to X B.
 * center, scale, impute, dtype: as mih_snp_create (they describe what the new handle presents).  reserve_bytes: the reserve of
 * device memory for fits on the new handle -- 0: mih_snp_create's rule, > 0: that many bytes, < 0: none (a row image of 125 GB that
 * only serves mih_xb_dense must not set aside 15.7 GB).
 * Memory: one more image of ceil(n / 32) ceil(p / 128) KB (about n p / 4 bytes), 24 bytes per sample and 4 per missing genotype for
 * the statistics and lists, and during the call 12 bytes per sample plus, with missing genotypes, 16 per SNP; the sum is compared
 * with the free memory before anything is allocated, and MIH_OOM names both byte counts.  The source is only read.  Only integer
 * atomics are used (counts, and an or of a constant per missing genotype): the result does not depend on the launch order.
 * Refusals: a handle that is not 2-bit, a dtype other than 64 / 32 (MIH_BAD_ARG); p >= 2^31 (MIH_BAD_DIM). */
int mih_snp_transpose(const mih_mat *src, int center, int scale, int impute, int dtype, int64_t reserve_bytes, mih_mat **out);
/* The genetic relationship (kinship) matrix of the samples of a 2-bit or a 16-bit dosage handle (a dense handle: MIH_BAD_ARG),
 * made entirely on the device -- SnpArrays.grm(x; method, minmaf) and the screen for pairs with Phi > 0.125 that
 * manuscript/UKBB_metabolomic/data_process.jl:80-103 runs between SnpArrays.filter and the principal components
 * (manuscript/NFBC_sim/NFBC_data_qc.jl:18-33 has GEMMA compute the same matrix).  Definitions (tests/grm_spec.py states them in
 * numpy): C the kept columns, m = |C|; mu_j and sinv_j exactly what mih_snp_mu_sigma returns for the handle, whatever its
 * center / scale / impute flags; c_ij = g_ij - mu_j for an observed genotype and 0 for a missing one (imputed by the mean;
 * a column whose genotypes are all missing has mu = NaN and contributes exactly 0).
 *   method 0, GRM:     Phi_ik = sum_{j in C} (c_ij sinv_j) (c_kj sinv_j) / (2 m): x_ij = c_ij sinv_j is the matrix a fit sees.
 *   method 1, Robust:  Phi_ik = sum_{j in C} c_ij c_kj / (2 sum_{j in C, mu_j finite} mu_j (1 - mu_j / 2)).
 * SnpArrays' third method, MoM, is not offered.  Float64 throughout on the f64 matrix pipe; every Phi_ik is summed over j in
 * ascending order by a schedule that the shapes alone fix (no atomics on the accumulator, no split over the columns), so
 * repeated calls agree bit for bit, whatever panel_cols; only the lower triangle is computed and the rest is its mirror
 * image, so Phi == Phi' bit for bit.  col_keep: p bytes 0 / 1 in host memory, NULL = all.  panel_cols: how many kept columns
 * are decoded to Float64 at a time, 0 = the library's rule (4096); a value that is not positive, or no multiple of 4, is
 * rounded up.  Device memory: 8 n_pad^2 bytes (n_pad = n rounded up to 128) for the accumulator, 8 n_pad panel_cols for the
 * panel, the lists; the sum is compared with the free memory before anything is allocated, and MIH_OOM names both byte
 * counts.  Everything is released before the call returns; the handle is only read.
 * mih_grm: phi receives the n x n matrix.
 * mih_grm_pairs: the pairs (i, k), i < k (0-based), with Phi_ik > threshold (strictly; a NaN Phi_ik is no pair), in the order
 * (i, k), so that no n x n array reaches the host.  *count = the pairs found; the first min(cap, *count) of them are written
 * to row_i, row_k, phi and nothing beyond (with cap = 0 the three may be NULL); diag (n, may be NULL) receives Phi_ii.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: a dense handle, an empty column selection, an unknown
 * method, cap < 0, a NaN threshold. */
int mih_grm(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double *phi /* n x n, host */);
int mih_grm_pairs(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double threshold,
                  int64_t cap, int64_t *row_i, int64_t *row_k, double *phi, int64_t *count /* pairs found, may exceed cap */,
                  double *diag /* n, may be NULL */);
/* The k leading eigenpairs of that Phi -- the principal components of the standardised genotype matrix, as PLINK and GCTA
 * compute them, which data_process.jl:103-110 hands to the fit as covariates -- without Phi leaving the device.  h, col_keep,
 * method and panel_cols are mih_grm's.  values (k): the k largest eigenvalues, descending; vectors (n x k, column-major):
 * vectors[i * n ..] is the unit eigenvector of values[i], its entry of largest magnitude (the lowest index on a tie) positive;
 * residuals (k): |Phi u_i - lambda_i u_i|_2 as the device evaluated it for the returned pair; *converged = max_i residuals[i] <=
 * tol * values[0]; *iters = products Phi Q taken.  Reaching max_iter is no error: the last Ritz pairs come back with
 * *converged = 0 and their residuals.
 * The method (tests/pca_spec.py states it in numpy): Phi, mirrored to the full symmetric n_pad x n_pad matrix, stays in device
 * memory; a blocked subspace iteration with a block of b = block columns, 0 = round_up(max(2 k, k + 8), 16), at most n --
 * a start hashed from (seed, row, column), Y = Phi Q on the f64 matrix pipe, Rayleigh-Ritz on Q'Y, and Q <- orth(orth(Y))
 * through the eigen-decomposition of Y'Y, which drops a direction with d_i <= 2^-52 d_1 for the rest of the run.  The b x b
 * algebra is the host's.  Every sum runs in an order the shapes fix, without atomics: the same arguments give the same bits,
 * whatever panel_cols; another seed or block gives the same pairs within the tolerance, not bit for bit.
 * Device memory: mih_grm's plus 8 (3 n_pad b + (n_pad / 512 + 4) b^2) bytes, checked in the same way before anything is
 * allocated (MIH_OOM names both byte counts): 8 n_pad^2 bytes bound the route to about 170 000 samples on a 288 GB device.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_grm refuses; k < 1 or k > min(n, 64); block
 * not 0 and (< k or > 128); tol not finite or negative; max_iter < 1; a null result pointer.  MIH_BAD_ARG, too, with nothing
 * written, when fewer than k directions survive: the message names the numerical rank found. */
int mih_grm_eig(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, int32_t k, int32_t block, double tol,
                int32_t max_iter, uint64_t seed, double *values /* k */, double *vectors /* n x k, column-major */,
                double *residuals /* k */, int32_t *iters, int32_t *converged);
/* Linear solves with the variance matrix of a mixed model on that Phi, V = tau_e I + tau_g Phi (tau_e > 0, tau_g >= 0): the
 * building block of the variance-component null model that SAIGE, fastGWA and GMMAT fit on related samples -- without Phi
 * leaving the device and without an n x n factorisation.  h, col_keep, method and panel_cols are mih_grm's.  B (n x m,
 * column-major, host, 1 <= m <= 128): the right-hand sides; X (n x m, column-major): X ~ V^-1 B.  Per column c: iters[c] the
 * iterations taken, converged[c] whether the recurrence residual reached |r|_2 <= tol |b|_2, residuals[c] the true residual
 * |b - V x|_2, formed explicitly with one more product.  Reaching max_iter is no error: the last iterate comes back with
 * converged[c] = 0 and its residual.  A zero column b gives x = 0, 0 iterations, converged.
 * The method (tests/lmm_spec.py states it in numpy): Phi, mirrored to the full symmetric n_pad x n_pad matrix, stays in device
 * memory; a conjugate gradient with the Jacobi preconditioner diag V = tau_e + tau_g Phi_ii from x = 0, every column with its
 * own scalars, V p once per iteration on the f64 matrix pipe; a column that has converged is frozen and the call ends when
 * all are, or at max_iter.  The scalars and the flags stay in device memory; every sum runs in an order that n_pad alone
 * fixes, without atomics: a column of X is bit for bit the same whatever the other columns of B, whatever m and panel_cols,
 * and on repeated calls.
 * Device memory: mih_grm's plus 8 (6 n_pad bp + n_pad + bp (n_pad / 16 + n_pad / 64 + 5)) + 4 (3 bp + 1) bytes, bp = m rounded
 * up to 16, checked in the same way before anything is allocated (MIH_OOM names both byte counts).
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_grm refuses; m < 1 or m > 128; tau_e not
 * finite or not positive; tau_g not finite or negative; tol not finite or negative; max_iter < 1; a null pointer. */
int mih_grm_solve(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double tau_e, double tau_g,
                  const double *B /* n x m, column-major */, int32_t m, double tol, int32_t max_iter,
                  double *X /* n x m, column-major */, int32_t *iters /* m */, int32_t *converged /* m */, double *residuals /* m */);
/* The variance-component null model of a mixed-model association scan for one Normal trait on that Phi, built once per call:
 * y = Z alpha + g + e, g ~ N(0, tau_g Phi), e ~ N(0, tau_e I), fitted by average-information REML as GMMAT and SAIGE do
 * (tests/lmm_spec.py states every step in numpy).  y (n), Z (n x c, column-major, full column rank, give the intercept), probes
 * Rademacher vectors for Hutchinson's trace estimates, 1 <= probes <= 64 and 1 + c + probes <= 128, hashed on the device from
 * (seed, row, probe).  Start: e0 the OLS residual, s2 = e0'e0 / (n - c), dbar = mean Phi_ii, tau = (s2 / 2, s2 / (2 dbar)).  An
 * iteration: S = V^-1 [y, Z, U] (one batched solve of mih_grm_solve's kind, tolerance cg_tol, at most cg_max_iter iterations),
 * Sigma = sym(Z'S_Z)^-1, P[y, U] = S - S_Z Sigma Z'S, a = Py, a second solve of [a, Phi a] and its projection; the score
 * (a'a - t_e, a'Phi a - t_g) / 2 with t_e = mean u'Pu, t_g = mean (Phi u)'Pu; the 2 x 2 average information
 * [a, Phi a]'[Pa, P Phi a] / 2, symmetrised; tau <- tau + 2^-h AI^-1 score with the smallest h >= 0 that keeps both components
 * at least a tenth of their previous values; converged when 2 max |tau'_i - tau_i| / (|tau'_i| + |tau_i|) <= tol_reml.  When
 * tau_g falls below 1e-8 s2 the fit ends on the boundary: tau_g = 0, tau_e = s2.  Then, at the final tau, alpha = Sigma Z'S_y
 * and Py.  G (n x R, column-major, 0 <= R <= 128; NULL with R = 0): mean-imputed genotype columns for the variance ratio of
 * GRAMMAR-Gamma / SAIGE, ratios[j] = g_j'P g_j / |(I - Z (Z'Z)^-1 Z') g_j|^2 by one more batched solve, *gamma their mean (NaN
 * for R = 0).  Outputs: tau (2: tau_e, tau_g), alpha (c), Py (n), trace (2: the last t_e, t_g), *dbar, tau_path (2 (max_iter + 1):
 * the start and every iterate, 2 (*iters + 1) numbers written), *iters, *state (1 converged, 2 boundary, 0 max_iter reached:
 * no error), *cg_iters (products V P over all solves), *worst_residual (the largest |b - V x| / |b| of any solve).  The n-sized
 * work is on the device; the c x c and 2 x 2 algebra is the host's.  The same arguments give the same bits, whatever panel_cols.
 * Device memory: mih_grm_solve's for m = max(1 + c + probes, R) plus 8 (5 n_pad bp + (n_pad / 512 + 4) bp^2) bytes, checked
 * before anything is allocated (MIH_OOM names both byte counts).
 * Refusals, MIH_BAD_ARG with nothing written: everything mih_grm refuses; c < 1, probes or R out of range; n <= c; a value of
 * y, Z or G that is not finite; a rank-deficient Z (the message names the rank); y in the span of Z; tolerances not finite
 * or negative; max_iter or cg_max_iter < 1; a null pointer; a kinship matrix whose mean diagonal is not positive; an
 * average-information matrix without a finite inverse. */
int mih_lmm_null(const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, const double *y, const double *Z, int32_t c,
                 int32_t probes, uint64_t seed, const double *G, int32_t R, double tol_reml, int32_t max_iter, double cg_tol,
                 int32_t cg_max_iter, double *tau, double *alpha, double *Py, double *gamma, double *ratios, double *trace,
                 double *dbar, double *tau_path, int32_t *iters, int32_t *state, int64_t *cg_iters, double *worst_residual);
/* out[i] = -log10 of the two-sided normal p-value of z[i], by the tail function every scan of this library uses (finite far
 * beyond where p underflows; NaN for a NaN): for a caller that rescales z after a scan, as the mixed-model scan does with the
 * variance ratio of mih_lmm_null.  Host code, no device call. */
int mih_neglog10p(const double *z, int64_t count, double *out);
/* The correlation of SNP pairs inside a window of columns (linkage disequilibrium) of a 2-bit handle and the pruning of its
 * columns by it, made on the device -- what `plink --indep-pairwise` does between SnpArrays.filter and the kinship matrix in
 * manuscript/NFBC_sim/NFBC_data_qc.jl:18-33; the mask goes to mih_grm / mih_grm_pairs / mih_grm_eig as col_keep.  Definitions
 * (tests/ld_spec.py states them in numpy): g_ij in {0, 1, 2} an observed genotype, miss(j) the missing rows of column j,
 * m_j = |miss(j)|, n_j = n - m_j, s_j = sum of the observed g_ij, mu_j = s_j / n_j whatever the handle's center / scale / impute
 * flags; t_ij = g_ij where observed and 0 where missing.  The LD of two columns is the correlation of the mean-imputed columns
 * (c_ij = g_ij - mu_j where observed, 0 where missing: the c_ij of mih_grm):
 *   D_jk = sum_i t_ij t_ik,  A_jk = sum_{i in miss(j)} t_ik,  M_jk = |miss(j) & miss(k)|            (integers, exact)
 *   C_jk = D_jk - mu_j (s_k - A_jk) - mu_k (s_j - A_kj) + mu_j mu_k (n - m_j - m_k + M_jk),   C_jj = D_jj - s_j^2 / n_j
 *   r_jk = C_jk / sqrt(C_jj C_kk)
 * in Float64, the operations in this order, each rounded by itself.  A column is degenerate when n_j = 0 or n_j D_jj = s_j^2
 * (monomorphic among its observed genotypes), decided in integers; it has r = 0 with every column.  Without a missing genotype
 * in either column this is the r that --indep-pairwise thresholds; with missing genotypes PLINK takes the samples observed in
 * both columns, and this library imputes by the mean, as everywhere else.
 * The band holds the pairs j < k with k - j < w, w = min(window, p).  The integers come from the matrix cores: the tiles of
 * two column groups are the A and the B operand of the FP4 instruction as they are stored.  They are exact, so the results
 * are bit for bit the same whatever panel_cols and slice_rows, and on repeated calls.  panel_cols: the columns whose band is
 * on the device at a time, 0 = the library's rule (4096, fewer for a wide window), else rounded up to a multiple of 32.
 * slice_rows: the rows one f32 accumulator covers, rounded up to a multiple of 128 and never more than 2^22 -- up to there the
 * sums are exact, so a larger value is taken as 2^22; 0 = the library's rule: 2^22, fewer where a launch would have too few
 * work items to fill the device.
 * Device memory beyond the handle: a panel's mask image (1024 bytes per tile of its column groups and of those the window
 * reaches; none for a matrix without missing genotypes), its integer partial sums, its band, the pair list and 40 p bytes; the
 * sum is compared with the free memory before anything is allocated, and MIH_OOM names both byte counts.  Everything is
 * released before the call returns; the handle is only read.
 * mih_ld_band: r (p x (w - 1) doubles, host): r[j (w - 1) + d - 1] = r_{j, j + d}, NaN where j + d >= p.  stats (may be NULL):
 * the same shape x 4 int64, D_jk, A_jk, A_kj, M_jk of k = j + d (zeros where j + d >= p).  diag (p, may be NULL): D_jj.
 * mih_ld_pairs: the pairs j < k of the band with r_jk r_jk > threshold (strictly, on the Float64 product; 0-based), in the order
 * (j, k), so that no p x w array reaches the host.  *count = the pairs found; the first min(cap, *count) of them are written to
 * col_j, col_k, r and nothing beyond (with cap = 0 the three may be NULL).
 * mih_ld_prune: keep (p bytes) receives the 0 / 1 mask of the greedy pass over that list, run on the host (tests/ld_spec.py,
 * prune): degenerate columns are dropped first; for s = 0, step, 2 step, ... < p the window is the columns [s, min(s + w, p));
 * inside it i ascends over the kept columns and k over the kept columns above i; where r_ik^2 > threshold and maf(i) < maf(k),
 * i is dropped and its loop left, otherwise k is dropped (a tie keeps the earlier column).  maf = min(f, 1 - f) of the exact
 * counts, f = (n1 + 2 n2) / (2 (n0 + n1 + n2)).  *n_pairs (may be NULL) = the pairs above the threshold.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: a handle that is not 2-bit, window < 2, step < 1, a NaN
 * threshold, cap < 0, a null result pointer. */
int mih_ld_band(const mih_mat *h, int64_t window, int64_t panel_cols, int64_t slice_rows, double *r /* p x (w - 1), host */,
                int64_t *stats /* p x (w - 1) x 4, may be NULL */, int64_t *diag /* p, may be NULL */);
int mih_ld_pairs(const mih_mat *h, int64_t window, double threshold, int64_t panel_cols, int64_t slice_rows, int64_t cap,
                 int64_t *col_j, int64_t *col_k, double *r, int64_t *count /* pairs found, may exceed cap */);
int mih_ld_prune(const mih_mat *h, int64_t window, int64_t step, double threshold, int64_t panel_cols, int64_t slice_rows,
                 uint8_t *keep /* p bytes */, int64_t *n_pairs /* may be NULL */);
/* The marginal association scan: a GLM score test of every column of a matrix by itself, given the null model of the covariates
 * -- the single-SNP analysis every paper of the reference compares IHT against -- made on the device for a 2-bit, a dosage or a
 * dense handle.  Definitions (tests/assoc_spec.py states them in numpy): x_ij the entry of the matrix as mih_xtv multiplies it
 * (the handle's center / scale / impute flags apply); A (n x t, column-major, 1 <= t <= 32) the score residuals, one column per
 * trait; w (n) the working weights >= 0, NULL = all ones; Z (n x c, column-major, 1 <= c <= 64) the covariates.  The null fit
 * itself is the caller's (GLM.jl; mendeliht's fit_null): A = (y - mu) mu'(eta) / (phi var(mu)), w = mu'(eta)^2 / (phi var(mu)).
 *   U_js = sum_i x_ij A_is,   b_j = sum_i x_ij w_i Z_i. (c-vector),   Q_j = sum_i x_ij^2 w_i
 *   G = Z'WZ = L L' (unpivoted Cholesky, on the host, Float64),   V_j = Q_j - |L^-1 b_j|^2
 *   z_js = U_js / sqrt(V_j),  beta_js = U_js / V_j,  se_j = 1 / sqrt(V_j),  neglog10p_js = -log10 erfc(|z_js| / sqrt 2)
 * in Float64; u = L^-1 b_j is formed row by row (u_k = sum_{l <= k} Linv_kl b_l, l ascending), |u|^2 with k ascending, every
 * operation rounded by itself.  With an intercept in span(Z) and impute = 1 the statistic does not depend on center / scale.
 * neglog10p is evaluated on the host from z and stays finite where p itself underflows (|z| = 40 gives 349.14).
 * Degenerate columns get NaN in z, beta, se and neglog10p: a 2-bit column without an observed genotype or monomorphic among its
 * observed ones (decided in integers, from mih_snp_counts), and any column with V_j <= 0.
 * U and b come from the library's fused X'R pass over R = [A | w o Z] (t + c residuals, 19 a pass).  Q of a dosage or dense
 * handle is summed per column in a fixed order.  Q of a 2-bit handle is
 *   Q_j = x(0)^2 W0 + x(1)^2 W1 + x(2)^2 W2 + x(miss)^2 Wm,   x(g) = ((g - [center] mu_j) [scale] sinv_j), x(miss) with g = [impute] mu_j
 * (the sum from the left), W1 / W2 the weight of the rows with dosage 1 / 2, Wm of the column's missing rows, W0 = sum w - W1 -
 * W2 - Wm.  With w == NULL the four are the integer counts.  Otherwise the weights enter as fixed-point integers R_i = rint(w_i
 * 2^e), e = 53 - ilogb(max w) (so R_i < 2^54; quantum q = 2^-e, at most q / 2 per row, relative to max w), and W1, W2 come from
 * the matrix cores: the bit planes tile & 0x11111111 and tile & 0x22222222 of the stored genotypes are the FP4 numbers 0.5 [g = 1]
 * and 1.0 [g = 2], the 27 base-4 digits u in {0, 1, 2, 3} of R_i are the FP4 numbers u / 2, and one instruction sums a digit over
 * the rows of a class.  A row adds a multiple of 1/4, at most 1.5, so an f32 accumulator is exact up to floor(2^24 / 6) rows:
 * a row slice holds at most 21 845 tiles of 128 rows = 2 796 160 rows.  slice_rows is rounded up to a multiple of 128 and capped
 * there; 0 = the library's rule: that limit, fewer where a launch would have too few work items to fill the device.  Every slice
 * stores its per-digit sums as integers; they are added per digit in 64 bits and the digits recombined once, exactly, so W0, W1,
 * W2, Wm are the exact sums of the R_i rounded ONCE to Float64, and with them every output is bit for bit the same whatever
 * slice_rows and on repeated calls.  The weights have their own front end and no outlier side channel (the one of the residual
 * front end is bypassed): the quantisation error is relative to max w, which dominates Q_j.
 * All pointers are host pointers.  z, beta, neglog10p: p x t column-major; se: p.  wsum (may be NULL): p x 3, W1, W2, Wm of
 * column j in wsum[3 j ..] (NaN for a handle that is not 2-bit).
 * Device memory beyond the handle: A, Z, w, R, the fused pass's workspace, the results, and for a weighted 2-bit call 8 bytes
 * per row, 16 per row of digit planes and 8192 bytes per (column group, slice) of integer partial sums; the sum is compared
 * with the free memory before anything is allocated, and MIH_OOM names both byte counts.  Everything is released before the call
 * returns; the handle is only read.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: a null handle or result pointer, t or c out of range, a NaN,
 * infinite or negative weight, a non-finite entry of A or Z, Z'WZ not positive definite, slice_rows < 0. */
int mih_assoc_score(const mih_mat *h, const double *A /* n x t */, int32_t t, const double *w /* n, may be NULL */,
                    const double *Z /* n x c */, int32_t c, int64_t slice_rows, double *z /* p x t */, double *beta /* p x t */,
                    double *se /* p */, double *neglog10p /* p x t */, double *wsum /* p x 3, may be NULL */);
/* mih_assoc_score for ONE Bernoulli trait with the logit link, with a saddlepoint approximation (SPA) of the p-value beside the
 * normal one: with few cases and rare alleles the score statistic is skewed and the normal tail overstates significance by
 * orders of magnitude.  z, beta, se and neglog10p are mih_assoc_score's for t = 1, bit for bit.  tests/spa_spec.py states the
 * following in numpy.  A = y - mu and w = mu (1 - mu) of the caller's null fit (which makes Z'A = 0), eta (n) its linear predictor
 * h_i; mu_i = sigma(h_i).  Per column j, with U_j, b_j, V_j, z_j and Linv as above:
 *   alpha_j = Linv' (Linv b_j) = G^-1 b_j        (u = Linv b_j as above; alpha_k = sum_{l >= k} Linv_lk u_l, l ascending)
 *   c_i = x_ij - sum_k Z_ik alpha_jk              (k ascending from 0; the covariate-adjusted genotype)
 *   K(t)   = sum_i [softplus(h_i + c_i t) - softplus(h_i)] - t sum_i c_i mu_i
 *   K'(t)  = sum_i c_i [sigma(h_i + c_i t) - mu_i]
 *   K''(t) = sum_i c_i^2 sigma(h_i + c_i t) (1 - sigma(h_i + c_i t))
 * where, for x = h_i + c_i t, e = exp(-|x|) and r = 1 / (1 + e): sigma(x) = r (x >= 0) or e r, sigma (1 - sigma) = (e r) r,
 * softplus(x) = max(x, 0) + log1p(e) -- nothing overflows at any t; mu_i comes from the same expressions, so K'(0) = 0 term by
 * term.  q = U_j; the statistic ranges over [S_min, S_max] = [sum_i min(c_i, 0), sum_i max(c_i, 0)] - sum_i c_i mu_i.
 * A tail at target s != 0: solve K'(t_hat) = s; w = sign(t_hat) sqrt(2 (t_hat s - K(t_hat))), v = t_hat sqrt(K''(t_hat)),
 * r = w + log(v / w) / w; the tail is log Phi(-|r|) by the arithmetic of neglog10p.  The root: Newton from t = 0, safeguarded by
 * the bracket (lo, hi) of the signs of f = K'(t) - s seen so far -- a step that leaves it (or is NaN) becomes the midpoint where
 * both ends exist, and while the outer end is missing 2 t (1 or -1 from t = 0); it stops when |f| <= 2^-30 sqrt(V_j) and then
 * takes one more Newton step (v is first-order sensitive to t_hat), after at most 64 evaluations of (K', K''); K and K'' at
 * t_hat take one more pass.  A tail is ACCEPTED when the iteration converged, t_hat is finite, K''(t_hat) >= 2^-20 V_j and r is
 * finite, not 0 and has the sign of t_hat.  (The third: where every carrier is a case the statistic sits at the end of its
 * range, K' reaches s only as t -> infinity, the float iteration "converges" far out with K'' / V ~ 1e-11 and r means nothing.)
 * The column: state 0 (not tried) if it is degenerate or |z_j| < cutoff, neglog10p_spa = neglog10p.  Otherwise tail 0 has
 * target +|q| and tail 1 has -|q|; the one on the side of q is always computed, the other contributes exactly 0 and is not
 * computed if its target is >= S_max (tail 0) or <= S_min (tail 1).  Every computed tail accepted: state 1, neglog10p_spa =
 * -log10(exp(l_0) + exp(l_1)) formed as a log-sum-exp, finite where p underflows.  Any computed tail refused: state 2,
 * neglog10p_spa = neglog10p (the normal value, as SAIGE falls back).  t_hat (may be NULL): p x 2 column-major, the roots of
 * tail 0 and tail 1, NaN where a tail was not computed or did not converge.  cutoff >= 0; +inf tries no column.
 * On the device: the columns with |z_j| >= cutoff are compacted in column order, alpha_j is formed for them, and one 256-thread
 * workgroup owns a flagged column for the whole solve of both tails.  It reads the column through the handle's decode (2-bit,
 * dosage, dense f64 / f32) and forms c_i ONCE into a slab of n doubles of its own (at most 2048 workgroups run, each walks
 * several columns): an evaluation is then one 8-byte load, one exp and one division per row whatever c is, where forming c_i
 * anew would cost c + 1 loads and c multiply-adds per row in each of the dozen evaluations of a column.  Nothing is staged
 * in LDS by n; the one n-dependent path: a pass loads a thread's rows four at a time (its loads' latency bounds it otherwise) and
 * the last 0 .. 3 singly -- n <= 768 has single rows only, n >= 1024 both kinds in every thread -- adding in row order either way.  Every sum is taken per thread over its rows tid, tid + 256, ... in ascending
 * order and then over a fixed tree of the 256 partial sums, without atomics and with contraction off; the loop's control values
 * are the same in every lane.  All sums span the whole column inside one workgroup and U, b, V are bit-reproducible, so
 * neglog10p_spa, state and t_hat are bit for bit the same whatever slice_rows and on repeated calls.  The finish of a column
 * (w, v, r, the tail, the log-sum-exp) is made on the host from t_hat, K(t_hat), K''(t_hat) (csrc/spa_finish.h).
 * Device memory beyond mih_assoc_score's: 24 bytes per row (eta, mu, softplus(eta)), 8 (c + 11) bytes per column at most (the
 * flagged indices, alpha, the tails), and min(p, 2048) slabs of 8 n bytes; it is added to the scan's and compared with the free
 * memory before anything is allocated, MIH_OOM names both byte counts.  Everything is released before the call returns; the
 * handle is only read.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_assoc_score refuses (with t = 1), a null w,
 * eta, neglog10p_spa or state, a non-finite eta, a negative or NaN cutoff. */
int mih_assoc_score_spa(const mih_mat *h, const double *A /* n: y - mu */, const double *w /* n: mu (1 - mu) */,
                        const double *Z /* n x c */, int32_t c, const double *eta /* n */, double cutoff, int64_t slice_rows,
                        double *z /* p */, double *beta /* p */, double *se /* p */, double *neglog10p /* p */,
                        double *neglog10p_spa /* p */, uint8_t *state /* p */, double *t_hat /* p x 2, may be NULL */);
/* mih_assoc_score for ONE Bernoulli trait with the logit link, with a Firth-penalised effect size and likelihood-ratio p-value
 * beside the score test's: beta = U / V is a one-step estimate, far from any likelihood estimate on a skewed column, and where
 * every carrier is a case the saddlepoint approximation is refused (state 2 above) and the maximum-likelihood estimate is
 * infinite.  This is the approximate Firth test of REGENIE: the covariates' effects are held at the null fit as an offset, and
 * the one-parameter logistic likelihood in the adjusted genotype, with Jeffreys' penalty, is maximised per column; the estimate
 * is finite under complete separation.  z, beta, se and neglog10p are mih_assoc_score's for t = 1, bit for bit.
 * tests/firth_spec.py states the following in numpy.  A, w, eta, c_i, h_i, mu_i, K, q = U_j and V_j are those of
 * mih_assoc_score_spa.  Per row, with x = h_i + c_i beta, e = exp(-|x|), r = 1 / (1 + e):
 *   sigma = r (x >= 0) or e r,   s = (e r) r,   d = (1 - e) r,   omega = -d (x >= 0) or d          (omega = 1 - 2 sigma)
 *   K1 = sum c (sigma - mu)   K2 = sum (c c) s   K3 = sum ((c c) c) (s omega)   K4 = sum ((c c) (c c)) (s (1 - 6 s))
 * the first four derivatives of K: the one-parameter model has log-likelihood beta q - K(beta), score q - K1 and information K2,
 * so at beta = 0 it reproduces the scan's U and V.  The penalised log-likelihood relative to beta = 0 is
 *   L*(beta) = beta q - K(beta) + log(K2(beta) / K2(0)) / 2,
 * stationary where g(beta) = q,  g = K1 - (K3 / K2) / 2,  g' = D = K2 - ((K4 K2 - K3 K3) / (K2 K2)) / 2  (D := K2 where D is not
 * finite or not > 0).  The root: Newton from beta = 0 with slope D under the safeguard of the saddlepoint root above (bracket,
 * midpoint, doubling; |g - q| <= 2^-30 sqrt(V_j), then one more Newton step; at most 64 evaluations); an evaluation whose g - q is
 * not finite ends the column as not converged.  A root always exists: g - q has opposite signs at -inf and +inf.  One more pass at
 * beta_hat gives K(beta_hat) and K2(beta_hat); I0 is K2 of the first evaluation (beta = 0; the kernel's own sum, not V).
 *   dev = 2 (beta_hat q - K(beta_hat) + log(K2(beta_hat) / I0) / 2)   (negative: 0)
 *   beta_firth = beta_hat,   se_firth = 1 / sqrt(K2(beta_hat)),   neglog10p_firth = -log10 erfc(sqrt(dev / 2))   (as neglog10p of z = sqrt dev)
 * firth_state: 0 (not tried) if the column is degenerate or |z_j| < cutoff; 1 if the iteration converged, beta_hat and dev are
 * finite and K2(beta_hat) is finite and >= 2^-40 V_j; 2 otherwise.  In states 0 and 2 the three Firth outputs are beta, se and
 * neglog10p bit for bit.  beta_firth is per unit of the entry x_ij, like beta.  firth_evals (may be NULL): the evaluations of
 * (K1 .. K4) a column took, 0 where it was not tried.  cutoff >= 0; +inf tries no column.
 * neglog10p_spa != NULL: the saddlepoint pass of mih_assoc_score_spa runs on the same selection (the same cutoff) in the same
 * call; spa_state is then required, t_hat may be NULL, and the three are bit for bit those of mih_assoc_score_spa.
 * neglog10p_spa == NULL: no saddlepoint pass, spa_state and t_hat are not touched.
 * On the device: the selection, alpha and the slabs of c_i are those of mih_assoc_score_spa, held once for both passes; one
 * 256-thread workgroup owns a flagged column for the whole solve, an evaluation is one 8-byte load beside eta_i and mu_i, one exp
 * and one division per row and carries four sums, each taken per thread over its rows tid, tid + 256, ... in ascending order
 * (four rows' loads ahead from n = 769 on) and then over a fixed tree, without atomics and with contraction off; the control
 * values are the same in every lane.  All Firth outputs, firth_evals included, are bit for bit the same whatever slice_rows and
 * on repeated calls.  The finish of a column is made on the host (csrc/firth_finish.h).
 * Device memory beyond mih_assoc_score's: what mih_assoc_score_spa needs without its tails (with them where the saddlepoint pass
 * runs too) and 56 bytes per column for the roots; the sum is compared with the free memory before anything is allocated,
 * MIH_OOM names the byte counts.  Everything is released before the call returns; the handle is only read.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_assoc_score_spa refuses (spa_state only where
 * neglog10p_spa is given), a null beta_firth, se_firth, neglog10p_firth or firth_state. */
int mih_assoc_score_firth(const mih_mat *h, const double *A /* n: y - mu */, const double *w /* n: mu (1 - mu) */,
                          const double *Z /* n x c */, int32_t c, const double *eta /* n */, double cutoff, int64_t slice_rows,
                          double *z /* p */, double *beta /* p */, double *se /* p */, double *neglog10p /* p */,
                          double *beta_firth /* p */, double *se_firth /* p */, double *neglog10p_firth /* p */,
                          uint8_t *firth_state /* p */, int32_t *firth_evals /* p, may be NULL; 0 where not tried */,
                          double *neglog10p_spa /* p, may be NULL: no saddlepoint pass */, uint8_t *spa_state /* p */,
                          double *t_hat /* p x 2, may be NULL */);
/* Gene-based burden and SKAT tests of sets of columns on top of the marginal scan, one trait, every handle kind (csrc/assoc_sets.hip;
 * tests/sets_spec.py states the same in numpy).
 * Inputs: A (n), w (n or NULL: ones), Z (n x c) and slice_rows exactly as mih_assoc_score takes them with t = 1.  nsets sets in CSR
 * form: set_ptr (nsets + 1, starting at 0, non-decreasing), set_col (0-based column indices) and omega (one variant weight per
 * entry, finite, >= 0).  Within a set the columns are strictly ascending and there are at most 128 of them; sets may overlap.
 * The scan: U_j, b_j, Q_j, V_j, z_j, the degenerate rule, G = L L' and u_j = L^-1 b_j are mih_assoc_score's, computed by the same
 * code; z, beta, se and neglog10p (p each) are its outputs bit for bit.
 * Members of a set: its entries whose column is not degenerate and whose omega > 0, in entry order; m_used is their count m.
 * Per set, over the members:
 *   C_jk = sum_i w_i x~_ij x~_ik (j > k), x~ as mih_xtv multiplies it (the handle's centre, scale and impute flags, a missing entry
 *          as the flags say) -- ONE chain of fused multiply-adds over the rows in ascending order, x~_ij w_i rounded first
 *   K_jk = C_jk - sum_l u_jl u_kl (l ascending from 0.0, every operation rounded by itself);  K_jj = V_j, the scan's own value;
 *          K mirrored to a full symmetric matrix
 *   M_jk = (omega_j K_jk) omega_k for j >= k, mirrored
 * Burden: a_j = omega_j U_j;  T = sum_j a_j;  rs_j = sum_k M_jk (k ascending), S = sum_j rs_j (j ascending);
 *   burden_z = T / sqrt(S), NaN where S <= 0;  neglog10p_burden its two-sided normal tail (normal_tail.h).
 * SKAT: skat_q = Q = sum_j a_j a_j;  lambda = the eigenvalues of M in descending order, every lambda_i <= 0 set to 0 (Jacobi on the
 *   device, not bit-identical to another solver: within |M|_F m 2^-52 of the exact ones);  the p-value is P(sum lambda_i chi2_1 > Q) by
 *   the saddlepoint approximation of Kuonen (1999):  K(t) = -1/2 sum log1p(-2 lambda_i t),  K' = sum lambda_i / (1 - 2 lambda_i t),
 *   K'' = 2 sum (lambda_i / (1 - 2 lambda_i t))^2,  t_hat solves K'(t_hat) = Q on t < 1 / (2 lambda_1),
 *   w = sign(t_hat) sqrt(2 (t_hat Q - K(t_hat))),  v = t_hat sqrt(K''(t_hat)),  r = w + log(v / w) / w,  the tail log Phi(-r).
 *   The root iteration, in units of 1 / (2 lambda_1) (s = 2 lambda_1 t, mu_i = lambda_i / lambda_1, q = Q / lambda_1,
 *   g(s) = sum mu_i / (1 - mu_i s), g2(s) = sum (mu_i / (1 - mu_i s))^2, w^2 = s q + sum log1p(-mu_i s), v = s sqrt(g2 / 2)):
 *   s = 0, lo missing, hi = 1 (the pole).  Repeat: evaluate g, g2 (one evaluation), f = g - q;  |f| <= 2^-40 q: converged,
 *   s_hat = s - f / g2 (one more Newton step), stop;  128 evaluations made: not converged, stop;  f < 0: lo = s, else hi = s;
 *   sn = s - f / g2;  if not lo < sn < hi:  f < 0: sn = (s + hi) / 2;  f > 0: sn = (lo + s) / 2 if lo exists, else 2 s if s < 0, else -1;
 *   s = sn.
 * skat_state, decided in this order, and neglog10p_skat:
 *   0  m = 0, or lambda_1 is not > 0 and finite: NaN
 *   2  rank one, m = 1 or lambda_2 <= 2^-40 lambda_1: the exact chi2_1 tail of Q / lambda_1, as the two-sided normal tail of
 *      sqrt(Q) / sqrt(lambda_1) -- a one-variant set with omega = 1 reproduces the scan's neglog10p bit for bit
 *   4  Q <= 0: 0
 *   5  the root iteration did not converge in 128 evaluations: the one-sided tail of the moment-matched normal
 *      z = (Q - sum lambda) / sqrt(2 sum lambda^2)
 *   3  near the mean, w^2 < 2^-40: the limit of r as w -> 0, r = kappa_3 / 6, kappa_3 = 8 sum lambda^3 / (2 sum lambda^2)^(3/2)
 *   1  the saddlepoint tail
 * A set without members has skat_q = 0 and NaN in burden_z and both p-values.
 * lambda (may be NULL) is laid out like set_col: the lambda of a set first, NaN after m_used.  cov (may be NULL): sum m_s^2 doubles,
 * m_s the entry count of set s (non-members included), each set's K over its entries in entry order, row-major, NaN in the rows
 * and columns of non-members.
 * Every set output is bit for bit independent of slice_rows, of the position of the set in the list and of the other sets.
 * Memory: everything the call allocates -- the scan's buffers, per set its K (m_s^2 doubles) and, for a set of more than 64
 * entries, a Jacobi slab ((m_s + 1)^2), the lists, u and the results -- is summed and compared with the free device memory before
 * anything is allocated; MIH_OOM names both counts.  Everything is released before the call returns; the handle is only read.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_assoc_score refuses at t = 1, a null m_used,
 * burden_z, neglog10p_burden, skat_q, neglog10p_skat or skat_state, nsets < 0, a null set_ptr, a set_ptr that does not start at 0 or
 * decreases, a set of more than 128 entries, null set_col or omega with entries, a column outside [0, p), columns of a set not
 * strictly ascending, an omega that is negative or not finite.  nsets = 0 is valid and returns the scan alone.
 * Not offered: ACAT, saddlepoint-adjusted variances for unbalanced case-control sets, collapsing of ultra-rare variants,
 * sets of more than 128 entries. */
int mih_assoc_sets(const mih_mat *h, const double *A /* n */, const double *w /* n, or NULL */, const double *Z /* n x c */, int32_t c,
                   int64_t slice_rows, int32_t nsets, const int64_t *set_ptr /* nsets + 1 */, const int32_t *set_col, const double *omega,
                   double *z /* p */, double *beta /* p */, double *se /* p */, double *neglog10p /* p */,
                   int32_t *m_used /* nsets */, double *burden_z /* nsets */, double *neglog10p_burden /* nsets */,
                   double *skat_q /* nsets */, double *neglog10p_skat /* nsets */, uint8_t *skat_state /* nsets */,
                   double *lambda /* like set_col, may be NULL */, double *cov /* sum m_s^2, may be NULL */);
/* mih_assoc_sets with SKAT-O on top: the optimal combination of the burden and the SKAT test of every set (Lee, Wu and Lin 2012;
 * csrc/assoc_skato.hip, csrc/skato_tail.h; tests/skato_spec.py states the same in numpy).  Every argument and output of
 * mih_assoc_sets keeps its meaning and its bits.  The grid: nrho values rho_1 < ... < rho_R in [0, 1], 1 <= nrho <= 16;
 * rho = NULL is SKAT's optimal.adj grid 0, 0.01, 0.04, 0.09, 0.16, 0.25, 0.5, 1 and needs nrho = 8.  A value above 0.999 is used as
 * 0.999, as SKAT does.
 * Per set with m members, M, rs_j = sum_k M_jk, S, T, Q as above, and per rho:
 *   Q_rho = (1 - rho) Q + rho (T T)
 *   M_rho = R_rho^1/2 M R_rho^1/2, R_rho = (1 - rho) I + rho 11', formed without a factorisation: c = sqrt(1 - rho),
 *           d = (sqrt((1 - rho) + m rho) - c) / m,  M_rho[j, k] = ((c c) M_jk + (c d) (rs_j + rs_k)) + (d d) S for j >= k, mirrored.  At
 *           rho = 0, c = 1 and d = 0 exactly: M_0 is M and its eigenvalues are `lambda` bit for bit (the same Jacobi code).
 *   lambda^(rho): the eigenvalues of M_rho, descending, every value <= 0 set to 0;  p_rho: the saddlepoint tail of
 *           (lambda^(rho), Q_rho) with the states of skat_state -- neglog10p_rho, and at rho = 0 neglog10p_skat bit for bit
 *   p_min = min_rho p_rho;  skato_rho = its rho as the caller gave it (a tie goes to the smaller rho)
 *   q_rho: tail_rho(q_rho) = p_min.  For skato_rho it is Q_rho.  For a rank-one lambda^(rho) it is lambda_1 z^2, z the two-sided
 *           normal quantile of p_min (bisection on neglog10p_of_z).  Otherwise the saddlepoint is inverted in its own parameter
 *           s = 2 lambda_1 t: q = lambda_1 g(s), log tail = log Phi(-r(s)); in y = 1 / (1 - s), F(y) = log tail - log p_min:
 *           a = 1 / (1 - s_rho) (the saddlepoint of Q_rho); |F(a)| <= 2^-40 |log p_min| or F(a) < 0: take a.  b = 2 a; while F(b) > 0:
 *           a = b, b = 2 b.  Then the Illinois rule: y = b - F(b) (b - a) / (F(b) - F(a)), the midpoint if that is not inside (a, b);
 *           |F(y)| <= 2^-40 |log p_min|: converged; F(y) > 0: a = y, and F(b) is halved if a moved the last time too; else b = y, and
 *           F(a) is halved likewise; b - a <= 2^-40 b: converged too, with this y.  128 evaluations of F in all: not converged.
 *   M~ = M - rs rs' / S (entry j >= k: M_jk - (rs_j rs_k) / S, mirrored), lambda~ its eigenvalues (values <= 0 set to 0);
 *   mu = sum lambda~,  v_xi = 4 (rs' M~ rs) / S (not below 0),  v = 2 sum lambda~^2 + v_xi,  tau_rho = rho S + (1 - rho) (rs' rs) / S
 *   delta(x) = min_rho (q_rho - tau_rho x) / (1 - rho),  delta'(x) = (delta(x) - mu) sqrt((v - v_xi) / v) + mu,  u0^2 = min_rho q_rho / tau_rho
 *   p = 2 int_0^u0 S~(delta'(u^2)) phi(u) du + 2 Phi(-u0),  S~ the saddlepoint tail of lambda~, 1 where delta' <= 0.  (x = u^2 removes
 *           the singularity of the chi2_1 density; beyond u0 the integrand is that density exactly, so nothing is truncated.)
 *   The integral: 16 panels of [0, u0], the 16-point Gauss-Legendre rule in each, one node per thread; every term a logarithm
 *           (log weight + log S~ + log phi + log(h / 2), h the panel's width), combined by a fixed pairwise log-sum-exp tree.  delta
 *           has up to R - 1 kinks where the minimising rho changes; the panels are cut there.  The kinks: with
 *           a_rho = q_rho / (1 - rho), b_rho = tau_rho / (1 - rho), a walk along the lower envelope of the lines a - b x from the line
 *           lowest at x = 0 (the steepest among equals); the next kink is the nearest crossing ahead with a steeper line (the
 *           steepest among equals), until u0^2.  The panels: the segments between 0, the kinks (as u = sqrt x) and u0 get one panel
 *           each, the remaining ones go one at a time to the segment whose panels are widest (the first among equals); a
 *           segment's panels are equal.  The device's libm is not the host's: the value agrees with tests/skato_spec.py to a
 *           tolerance, and is the same bits for every slice_rows, position of the set and list of other sets.
 * skato_state and neglog10p_skato:
 *   0  no value: m = 0, S <= 0 (or NaN), skat_state 0, or a p_rho without a value: NaN
 *   2  rank one: m = 1 or skat_state 2: neglog10p_skat bit for bit (skato_rho is NaN)
 *   4  fallback: a p_rho came from state 4 or 5, p_min = 1, a quantile did not converge or the integral is not a number:
 *      min(1, R p_min)
 *   1  the integral's value
 *   3  clamped: the integral left [p_min, R p_min] and was moved to the nearer end (SKAT's own rule)
 * neglog10p_rho (nsets x nrho, row-major, may be NULL).  lambda_rho (may be NULL): nrho + 1 arrays laid out like set_col, one after
 * the other: lambda^(rho_1) .. lambda^(rho_R), then lambda~; NaN after m_used.
 * Memory: beside mih_assoc_sets's, nrho + 1 Jacobi slabs for every set of more than 64 entries, lambda_rho and the integrands, all
 * counted in the same check before anything is allocated.
 * Refusals, MIH_BAD_ARG with nothing allocated and nothing written: everything mih_assoc_sets refuses, a null neglog10p_skato,
 * skato_rho or skato_state, nrho < 1 or > 16, rho = NULL with nrho != 8, a rho outside [0, 1] (or NaN), a grid not strictly
 * ascending. */
int mih_assoc_sets_skato(const mih_mat *h, const double *A /* n */, const double *w /* n, or NULL */, const double *Z /* n x c */, int32_t c,
                         int64_t slice_rows, int32_t nsets, const int64_t *set_ptr /* nsets + 1 */, const int32_t *set_col, const double *omega,
                         int32_t nrho, const double *rho /* nrho, or NULL: the default grid */,
                         double *z /* p */, double *beta /* p */, double *se /* p */, double *neglog10p /* p */,
                         int32_t *m_used /* nsets */, double *burden_z /* nsets */, double *neglog10p_burden /* nsets */,
                         double *skat_q /* nsets */, double *neglog10p_skat /* nsets */, uint8_t *skat_state /* nsets */,
                         double *lambda /* like set_col, may be NULL */, double *cov /* sum m_s^2, may be NULL */,
                         double *neglog10p_skato /* nsets */, double *skato_rho /* nsets */, uint8_t *skato_state /* nsets */,
                         double *neglog10p_rho /* nsets x nrho, may be NULL */, double *lambda_rho /* (nrho + 1) x entries, may be NULL */);
/* Re-expresses every non-missing numerator of a dosage handle over denom (a multiple of its denominator, at most 32767) and
 * recomputes the column statistics: the same matrix on a finer grid (column shards agree on one denominator this way).  Not
 * while a fit uses the handle. */
int mih_dosage_regrid(mih_mat *h, int32_t denom);
/* Numerators of columns [col0, col0 + ncols) of a dosage handle into out (n x ncols column-major, 0xFFFF = missing). */
int mih_dosage_export(const mih_mat *h, int64_t col0, int64_t ncols, uint16_t *out);
/* Releases the matrix.  A mih_session must not be stepped after its matrix is gone, but it may be destroyed later: the
 * reserve of device memory a large matrix keeps for its fits lives until its last user. */
int mih_mat_destroy(mih_mat *h);
/* The reserve of device memory a matrix keeps for the fits that run on it (lock-step workspaces, IHTVariable blocks: no fit then
 * calls hipMalloc / hipFree).  A 2-bit matrix of 4 GiB or more gets one when it is created; this call gives one to ANY 2-bit
 * matrix -- bytes = 0: sized from its dimensions by the library's rule, bytes > 0: that size -- or releases it (bytes < 0).
 * Not to be called while a fit is running on the matrix.  MIH_OOM if the device has less than four times the size free. */
int mih_mat_reserve(mih_mat *h, int64_t bytes);
/* The score image of a 2-bit matrix: a second, derived image of the (immutable) matrix that only the single-residual X'r pass
 * of a fit reads (residual format 428).  Columns with at most max_hom_fraction * n dosage-2 entries are stored at ONE bit per
 * genotype (the plane g >= 1) with the rows of their dosage-2 entries in side lists, the other columns as they are; the pass
 * over it gives bit for bit the results of the pass over the matrix and moves fewer bytes.  mode: MIH_IMAGE_BUILD builds it
 * (replacing an earlier one; max_hom_fraction <= 0: the library's default; MIH_BAD_ARG if no column qualifies), MIH_IMAGE_RELEASE
 * drops it, MIH_IMAGE_QUERY changes nothing; every mode then reports the image's bytes and its one-bit columns (0, 0: no image;
 * either pointer may be NULL).  The image is a cache: fits and sessions started while it exists use it and keep it alive while
 * they live; mih_device_trim, and any allocation of the library that runs out of device memory, release the images nobody uses.
 * An argument, not an environment switch. */
#define MIH_IMAGE_QUERY 0
#define MIH_IMAGE_BUILD 1
#define MIH_IMAGE_RELEASE 2
int mih_mat_score_image(mih_mat *h, int mode, double max_hom_fraction, int64_t *bytes, int64_t *class1_cols);
/* Releases every score image on the device that no live fit or session is using; released_bytes (may be NULL): how much. */
int mih_device_trim(int device, int64_t *released_bytes);
int mih_mat_dims(const mih_mat *h, int64_t *n, int64_t *p);
/* `x.μ`, `x.σinv` of the SnpLinAlg, or mu_j (dosage units) and 1/sigma_j (1 where sigma_j = 0) of a dosage handle */
int mih_snp_mu_sigma(const mih_mat *h, double *mu, double *sinv);
/* Re-encode the device matrix as PLINK .bed columns (ceil(n/4) bytes each): lets a
 * synthetic matrix be handed to any other PLINK consumer. */
int mih_snp_export_bed(const mih_mat *h, uint8_t *bed_cols_out);
/* naive_impute(x::SnpArray, destination) -- src/utilities.jl:862-899: the PLINK columns of the matrix with every
 * missing entry (0x01) replaced by the most frequent genotype of its SNP (ties: 0x02, then 0x03, then 0x00, the order
 * of the reference's if / elseif chain); non-missing entries are unchanged.  The caller writes the 3-byte .bed header. */
int mih_snp_naive_impute(const mih_mat *h, uint8_t *bed_cols_out);

/* ---- genotype linear algebra ---------------------------------------------- */
/* mul!(out, Transpose(x), r)  -- call site src/utilities.jl:133 (score!) */
int mih_xtv(const mih_mat *h, const double *r, double *out);
/* SnpArrays.mul!(p_by_r, Transpose(sla), n_by_r) -- call site src/multivariate.jl:85;
 * R is n x m column-major, OUT is p x m column-major. */
int mih_xtv_batched(const mih_mat *h, const double *R, int m, double *OUT);
/* The same with an explicit fixed-point format of the residuals.  A residual is scaled by a power of two, rounded to an
 * integer R and written as digits that FP6 / FP4 represent exactly; each digit plane is one column of the MFMA B operand,
 * the dot products with the dosages are exact, and the only rounding is that of the residual.  digits = base * 100 + digits:
 *   0 = library default: 4910 for every multi-residual context (this call, cv_iht, model paths, multivariate fits,
 *        init_beta) whatever the number of residuals, 428 for the workspace of a single univariate fit.
 *   4910 10 base-49 digits d/8 in FP6 (e2m3), |R| < 2^54: rounding 2^-54 max|r|, below that of an n-term f64 sum.  The digit
 *        columns of a pass's residuals are packed back to back over its 32-column operands (19 residuals in six operands).  Row slices of 2^18 rows; above 2^22 rows the default steps down to 1316.
 *   1316 16 base-13 digits d/2 in FP4 (e2m1), |R| < 2^57, two residuals per operand (2^20-row slices; above 2^24
 *        rows the default steps down to 428).
 *   428  28 base-4 digits {-2..1}/2 in FP4, |R| < 2^54, one residual per operand (the first format; cross-check).
 *   4908 8 base-49 FP6 digits, |R| < 2^43, FOUR residuals per operand: opt-in fast mode for fused multi-RHS
 *        passes (cv_iht, multivariate, init_beta); relative error of X'r about 2^-43 max|r| / |r|_rms ~ 1e-12.
 *   1308 8 base-13 FP4 digits, |R| < 2^27, four per operand (~15 % faster than 4908, error ~1e-7).
 * A result never depends on which other residuals share a pass or on the kernel shape, only on the format.
 * What the fixed point costs: the quantum is 2^-54 of the LARGEST entry the fixed point carries (2^-53 at worst), and the error of
 * a column's X'r is at most sum_i g_ij times that quantum (plus 64 ulp of the result for the f64 recombination) -- for residuals
 * without heavy tails tighter than an n-term f64 dot product.  Heavy tails (round 6, csrc/peel.h): rows whose |r_i| towers over the
 * rest -- max|r| > 64 x the lower quartile of the maxima of the 64 strided 256-row blocks, at most 64 such rows -- leave the fixed
 * point: their digits are zero, the scale is set by the largest of the REST, and k_xtv_finalize adds their terms g_ij r_i in f64
 * (m rows of the 2-bit matrix per column, only when the guard fires).  With one entry 1e8 or 1e12 x the rest every column, with or
 * without that row, is within 2 x 2^-53 sum_i g_ij |r_i| of the exact rational value (numpy's pairwise sum: 8 x) and within 1e-13 of
 * its own value unless that value has cancelled; a residual without such rows does not move a bit.  For n < 16384 with a short or
 * all-zero 256-row block (a single last row, the held-out rows of a contiguous fold) among the first few the guard's threshold is tiny or
 * 0 and it may fire on ordinary residuals -- up to 64 ordinary rows then ride the side channel, or none; the result keeps the accuracy
 * above either way (a cost, a rescan of the residual, not an error).  The side channel adds its terms in a compensated sum: one rounding
 * of the result for up to 64 rows.  What is left: more than 64 rows
 * above the guard's threshold (a heavy TAIL rather than a few outliers) keep the plain scale, i.e. entry r_i keeps
 * 54 + log2(|r_i| / max|r|) bits -- 200 rows 1e6 x the rest: ~1e-7 on the columns that carry none of them.  A Poisson fit with a
 * planted count of 500 among counts of ~1 keeps the CPU restatement's loglikelihood trace to 1e-12 over 172 steps.
 * The scale is 2^-e with e = ebits - ilogb(max|r| of the rows in the fixed point), ebits = 53 (4910, 428), 56 (1316), 42 (4908), 26 (1308),
 * capped at e = 1000 (a residual below 2^-947 is rounded to a quantum of 2^-1000); EVERY FINITE residual is scaled, up to max|r| = DBL_MAX
 * (before, max|r| >= 1e300 kept e = 0 and gave a finite, wrong row).  A column whose exact value overflows comes out as +-Inf or NaN.
 * A residual with a NaN or +-Inf entry, or whose sum overflows (two entries of 1.5e308), gives NaN in EVERY column of its row of OUT
 * (the reference's floating-point mul! gives NaN or +-Inf in every column that touches the entry -- all of them for a centered matrix);
 * the other residuals of the call are untouched.
 * (tests/test_gpu_linalg.py: test_xtv_fixed_point_under_adversarial_dynamic_range, test_peeled_rows_in_fused_passes_with_missing_genotypes;
 * tests/test_gpu_resident.py: test_poisson_fit_with_a_planted_count_outlier; tests/test_gpu_xtv_residual_edges.py: the guard, the scale
 * rule and the side channel at their edges, against exact values) */
int mih_xtv_batched_fmt(const mih_mat *h, const double *R, int m, int digits, double *OUT);
/* out = sum_t x[:, idx[t]] * val[t]  -- the column loops of update_xb!
 * (src/utilities.jl:98-106) and iht_stepsize! (:731-739); idx 0-based. */
int mih_xv_sparse(const mih_mat *h, const int64_t *idx, const double *val, int64_t nnz, double *out);
/* mul!(out, x, B) for a dense B: OUT (n x t, column-major) = X * B (p x t, column-major), X as the SnpLinAlg of `h` presents it, or
 * with the flags overridden (center / scale / impute: 0, 1, or -1 = the handle's).  rows: the handle mih_snp_transpose made from h
 * (any flags; its tiles and lists are what is read).  digits: as mih_xtv_batched_fmt.
 * X B = (X')' B: the X'r pass runs over the row image with the columns of a = sinv o B (B itself without scale) as its residuals --
 * the same exact fixed point, the same 19 fused operands (any t >= 1: the pass planner cuts it into passes), the same row slices
 * and outlier side channel -- on raw codes with missing = 0; then one thread per sample adds
 *     + sum_{j in miss(i)} mu_j a_jt   (impute: the sample's list of the row image, ascending j, one f64 chain)
 *     - sum_j mu_j a_jt                (center: c_t, a fixed tree over the SNPs, the same bits on every call)
 * in this order, every operation one f64 rounding (no contraction).
 * OUT[:, t] depends only on B[:, t], the two matrices and digits: not on which other columns share the call, not on the row slices or
 * any other internal of the pass, not on the number of calls.  Accuracy: the pass's own (above mih_xtv_batched_fmt) -- the main term
 * is within 2^-53 max_j |a_jt| sum_j code_ij + 64 ulp of the exact value -- plus the roundings of a, of mu a, of the chain (one per
 * missing SNP of the sample), of the tree (at most 19 + ceil(p / 262144) per term) and of the two final additions; tests/xb_spec.py
 * derives the elementwise bound.  A NaN or +-Inf anywhere in a column of B (or in its a), or a column whose sum overflows, gives NaN
 * in that whole column of OUT and leaves the other columns untouched: the pass's own rule.  A SNP without an observed genotype has
 * mu = NaN: with center or impute every entry of OUT is NaN, as every entry of that column of X is.
 * Memory: beside the row image (mih_snp_transpose), 8 t (3 p + n) bytes and the pass's workspace, released before the call returns.
 * Refusals (MIH_BAD_ARG, nothing written): a null pointer; h or rows not 2-bit (the products of dense and dosage handles are not
 * offered); rows that is not the image of h -- rows->n != h->p, rows->p != h->n, another device, another number of missing
 * genotypes: the message holds both shapes; t < 1; a flag outside -1, 0, 1; an unknown format. */
int mih_xb_dense(const mih_mat *h, const mih_mat *rows, const double *B, int32_t t, int center, int scale, int impute,
                 int digits, double *OUT);

/* ---- projections ----------------------------------------------------------- */
/* project_k!(x, k) src/utilities.jl:553-559: zero every |x_i| < |k-th largest|;
 * ties at the threshold are kept; *n_kept = number of non-zeros left. */
int mih_project_topk(double *x, int64_t len, int64_t k, int64_t *n_kept);
/* project_group_sparse!(y, group, J, k) src/utilities.jl:613-679; group labels 1..G, G = the largest
 * label in group.  k points to one entry, or, when k_is_vector, to at least G entries (k[g-1] for label
 * g; the call reads all G of them and nothing beyond, so a shorter buffer is the caller's error). */
int mih_project_group_sparse(double *y, const int64_t *group, int64_t len, int64_t J,
                             const int64_t *k, int k_is_vector);

/* ---- fit_iht ---------------------------------------------------------------- */
/* Column-sharded single fit (one process per GPU): every process owns a contiguous block
 * of the SNP columns as its own mih_mat; y, z and all n-vectors are replicated.  The reference has no
 * multi-device fit, so there is no line to cite for the exchange itself: the library calls back into
 * the host at the points where iht_stepsize!/update_xb! (src/utilities.jl:722-764, 93-118) sum over
 * the support columns (all-reduce of n+1 / n doubles on the device) and where project_k! (utilities.jl:553-559)
 * needs the global k-th largest entry (all-gather of 1 + 2K doubles per rank: the shards' candidates as
 * (global index, value) pairs, from which every rank also rebuilds the whole k-sparse model, so that _choose!
 * and check_convergence, utilities.jl:444-458, 953-957, need no exchange; with prior weights or ties beyond the
 * message size two scalar reductions remain).  The host implements the
 * two collectives with its own communicator (RCCL through torch.distributed in the Python mirror,
 * MPI.Allreduce in the Julia glue).  Both must return 0 on success, on every rank, in the same order. */
typedef struct mih_comm {
    int32_t rank, world;
    int64_t col_offset;       /* global 0-based index of this shard's first column */
    int64_t p_global;         /* total number of SNP columns over all shards */
    /* in-place reduction of `count` doubles over the ranks; op 0 = sum, 1 = max.  on_device = 1: buf is
     * device memory on the fit's GPU and everything queued on the fit's stream has completed; the
     * callback returns after the reduced values are visible to any stream. */
    int (*allreduce)(void *user, double *buf, int64_t count, int32_t op, int32_t on_device);
    /* recv[r*count .. (r+1)*count) = `send` of rank r; host memory */
    int (*allgather)(void *user, const double *send, int64_t count, double *recv);
    void *user;
} mih_comm;

/* A native exchange for the column-sharded fit: an RCCL communicator owned by the library, whose two callbacks run
 * ncclAllReduce / ncclAllGather on a private stream (xGMI between the GPUs of a node) without re-entering the host
 * language.  One process per GPU.  Rank 0 calls mih_rccl_unique_id and hands the 128 bytes to the other ranks by whatever
 * the launcher offers (MPI_Bcast, torch.distributed.broadcast, a file); every rank then calls mih_comm_create_rccl and
 * passes the returned mih_comm in mih_fit_params::comm (and frees it with mih_comm_destroy_rccl).  librccl is loaded on
 * first use (dlopen; MENDELIHT_RCCL_LIB overrides the name).  No reference counterpart: the reference has no multi-device fit. */
int mih_rccl_unique_id(void *id128);
int mih_comm_create_rccl(const void *id128, int32_t rank, int32_t world, int32_t device, int64_t col_offset,
                         int64_t p_global, mih_comm **out);
/* diagnostics: the rank count RCCL itself reports for the communicator (ncclCommCount; -1 if unavailable) and the librccl file that
 * was loaded (a process may hold two: comm.hip picks the one beside its own libamdhip64) */
int mih_comm_info(const mih_comm *c, int32_t *ranks_seen, char *librccl_path, int64_t cap);
int mih_comm_destroy_rccl(mih_comm *c);
/* The ONE exchange of a cross-validation run by one process per GPU (the reference combines its threads' losses in the shared
 * `mses` vector, cross_validation.jl:99,113,124-127): every rank passes the nfolds * npath losses mih_cv_iht / mih_cv_mv /
 * mih_fit_iht_path left it (zeros for the combinations of other ranks); on return every rank holds their sum over the ranks
 * = the complete matrix, ready for mih_cv_meanloss.  One all-gather through `c` (ncclAllGather over xGMI for a communicator
 * made by mih_comm_create_rccl -- col_offset / p_global play no role here, pass 0 and 1 -- or the caller's own callbacks),
 * summed in rank order.  No MPI, no host-language collective. */
int mih_cv_allgather(const mih_comm *c, double *mses_raw, int64_t count);

/* keyword arguments of fit_iht (src/fit.jl:64-81) */
typedef struct mih_fit_params {
    int64_t  k;               /* sparsity (ignored when ks != NULL) */
    int64_t  J;               /* max groups */
    int32_t  dist, link;      /* MIH_NORMAL.., MIH_IDENTITY.. */
    double   nb_r;            /* NegativeBinomial r (d.r) */
    double   tol;
    int32_t  max_iter, min_iter, max_step;
    int32_t  est_r;           /* MIH_ESTR_* */
    const uint8_t *zkeep;     /* q flags or NULL = trues(q) */
    const double  *weight;    /* p prior weights or NULL */
    const int64_t *group;     /* p group labels (1-based) or NULL */
    const int64_t *ks;        /* per-group sparsity (k::Vector{Int}) or NULL */
    int64_t  nks;
    /* per-iteration callback = the `verbose` line of fit.jl:194-196; may be NULL */
    void (*progress)(void *user, int iter, double logl, int backtracks, double tol);
    void    *progress_user;
    int32_t  init_beta;       /* fit.jl:80 init_beta: start from the p univariate regressions
                                 (initialize_beta!, src/utilities.jl:776-812; Normal only) */
    const mih_comm *comm;     /* NULL = single process; else this process's shard of a column-sharded
                                 fit: h, weight, res->beta (mih_mv_result::B) cover the LOCAL columns only (mih_fit_iht,
                                 mih_session_* and mih_fit_mv; no cross-validation; init_beta for the univariate fit only.
                                 Round 6, univariate fit: debias -- the support's n x k panel is summed over the shards, one
                                 all-reduce of n * k doubles per refit, and every shard runs the same refit -- and the group
                                 projection: `group` holds the labels 1..G of the LOCAL columns (G, J, k and a vector k are
                                 the whole matrix's), every shard sends its own k_g largest of each group -- two all-gathers
                                 per projection -- and walks the union by the reference's rule) */
    int32_t  debias;          /* fit.jl:73,188 debias: after a step (iter >= 5) that kept the support, refit the
                                 support columns by GLM (debias!, src/utilities.jl:1014-1020; the reference needs
                                 memory_efficient=false for it, the device builds the n x k panel on the fly) */
    int32_t  xtv_digits;      /* fixed-point format of the residual in this call's X'r passes (no reference counterpart):
                                 0 = library default; 4910, 4908, 1316, 1308, 428 -- see mih_xtv_batched_fmt.  A property
                                 of the CALL: concurrent fits on one matrix may use different formats.
                                 -1 = auto, for the lock-step drivers (mih_cv_iht, mih_fit_iht_path) with a GLM link
                                 (Bernoulli / Poisson / NegBin / Gamma / InverseGaussian: the reference tolerance there is
                                 1e-4): every residual is looked at on its own -- if max |r| <= 128 rms(r) it is scored in the
                                 43-bit format (4908: four residuals per operand, ~19 % less pass time at configs[3]; its
                                 rounding then stays ~1e-11 of a column's X'r), otherwise in the 54-bit format.  The choice
                                 depends on that residual alone, so a fit still gives the same bits whatever its company.
                                 mih_fit_mv: per X'R pass, the 43-bit format when EVERY trait's row of T1 = Gamma * resid passes
                                 that test (three operands instead of four at r = 10), else the 54-bit one; one more small
                                 readback per iteration.  Univariate Normal fits, single fits and mih_cv_mv: as 0. */
    /* The reference's RANDOM tie-break, _choose! (src/utilities.jl:444-458, src/multivariate.jl:310-351): when a projection
     * leaves more than k non-zero effects (exact ties in |b|) the reference removes the excess at random with the caller's
     * RNG.  NULL: the library removes the smallest |b| (ties: highest index) and raises choose_fired in the result.
     * Otherwise the library asks the caller, so a Julia binding that answers with the reference's own two calls reproduces
     * the reference's draw from the same RNG state (the only RNG use on the path besides the default `folds`):
     *   kind MIH_CHOOSE_SAMPLE    `sample(non_zero_idx, excess, replace=false)` (utilities.jl:453): list = the n positions of
     *                             non-zero SNP effects (findall order, 0-based); write the `excess` positions to zero to out.
     *   kind MIH_CHOOSE_SHUFFLE_B `shuffle!(B_nz_idx)` (multivariate.jl:336): list = the n linear indices (trait + r * SNP,
     *                             eachindex order) of the non-zero entries of B; write ALL n in shuffled order to out.
     *   kind MIH_CHOOSE_SHUFFLE_C `shuffle!(C_nz_idx)` (multivariate.jl:337), called right after _B: the non-zero entries of
     *                             the covariates NOT in zkeep (trait + r * covariate); write all n in shuffled order to out.
     * An EMPTY list is not handed over (shuffle! of an empty vector draws nothing from the RNG).
     * The library then zeroes what the reference's loop zeroes (multivariate.jl:338-348).  Called on the thread that called
     * mih_fit_iht / mih_session_* / mih_fit_mv (a session keeps the pointer: it must stay valid until mih_session_destroy);
     * a non-zero return aborts the fit with MIH_BAD_ARG.  Ignored by the lock-step
     * drivers (cv_iht, model paths: their fits run on the library's threads -- the reference's own threaded loop draws from
     * task-local RNGs there) and by column-sharded fits (comm != NULL). */
    int (*choose)(void *user, int32_t kind, const int64_t *list, int64_t n, int64_t excess, int64_t *out);
    void    *choose_user;
    /* mih_cv_iht with est_r != MIH_ESTR_NONE only.  The reference keeps one IHTVariable per Julia thread and re-uses it for every
     * (fold, k) combination `Threads.@threads :static` hands that thread (cross_validation.jl:91,100-110): the NegBin r left by
     * one fit is where the thread's next fit starts, so the losses depend on JULIA_NUM_THREADS.  cv_threads = that number: the
     * fold-major combinations are cut into cv_threads contiguous blocks (the first total % cv_threads one longer, as :static
     * does), each block is a chain of fits handing r on, and the chains advance in lock-step.  0 or 1 = ONE chain over the whole
     * grid: what the reference does at its default Threads.nthreads() == 1, and what both bindings (and the tests' CPU checker) mean by the
     * same value; nfolds = one chain per fold (five times faster at configs[3]'s shape: an explicit choice, because
     * the losses differ from a default reference run).  With world > 1 chain c is
     * evaluated by rank c mod world (mih_cv_assignment does not apply).  Ignored without est_r: those fits are independent. */
    int32_t  cv_threads;
    /* How iht_one_step! (fit.jl:213-263) is driven.  0 = the step is resident on the device wherever the fit allows it (a plain 2-bit
     * univariate fit: no group projection, est_r or debias; a column shard only over the library's own communicator,
     * mih_comm_create_rccl, whose collectives are then queued inside the chain): the k-sparse iterate, the exact finish of project_k!,
     * the backtracking decision and the stopping rule live in device memory, the host queues the kernels of a step without
     * waiting and reads one record per series of attempts, one step behind.  Exact ties that need _choose! hand the step back to the host-driven
     * path.  Since round 6 also the fits of the lock-step drivers (mih_cv_iht, mih_fit_iht_path: a fit queues its step behind its lane's
     * fused pass and reads one record per step) and models of up to ~8000 effects (k_res_select_big; ~2000 before).
     * 1 = every step host-driven (rounds 1-4: 26 launches, three waits).  Same results either way, bit for bit. */
    int32_t  step_mode;
} mih_fit_params;
enum { MIH_CHOOSE_SAMPLE = 0, MIH_CHOOSE_SHUFFLE_B = 1, MIH_CHOOSE_SHUFFLE_C = 2 };

/* IHTResult (src/data_structures.jl:245-256) + the per-iteration log */
typedef struct mih_fit_result {
    double   time;            /* seconds inside the fit loop (fit.jl:157,200) */
    double   logl;            /* best loglikelihood */
    int64_t  iter;
    double   pve;             /* sigma_g (src/pve.jl:32) */
    double   nb_r;            /* final NegBin r */
    int32_t  choose_fired;    /* 1 if the reference's RNG tie-break _choose! would have run */
    int32_t  n_trace;
    double  *beta;            /* caller-allocated p  (best_b) */
    double  *c;               /* caller-allocated q  (best_c) */
    double  *logl_trace;      /* caller-allocated max_iter doubles, or NULL */
    double  *tol_trace;       /* "                                      */
    int32_t *bt_trace;        /* caller-allocated max_iter int32,  or NULL */
    double  *mu;              /* caller-allocated n (final v.mu), or NULL */
} mih_fit_result;

/* fit_iht(y, x, z; ...) src/fit.jl:60-118 (always the memory_efficient=true formulation: no dense
 * n x k copy of the support is kept).  z is n x q column-major (first column all ones);
 * train is NULL (all samples) or n flags = cv_train_idx. */
int mih_fit_iht(const mih_mat *h, const mih_fit_params *prm, const double *y,
                const double *z, int64_t q, const uint8_t *train, mih_fit_result *res);

/* cv_iht(y, x, z; path, q, folds, ...) src/cross_validation.jl:60-131.
 * folds: n labels in 1..nfolds.  The (fold,k) combinations are enumerated
 * fold-major (cross_validation.jl:217-223); this call evaluates those that
 * mih_cv_assignment gives to `rank` and writes their held-out deviance sums into
 * mses_raw[nfolds*npath] (others left 0), so ranks combine with ONE sum-reduce /
 * gather.  mih_cv_meanloss then applies meanloss (:304-320). */
int mih_cv_iht(const mih_mat *h, const mih_fit_params *prm, const double *y,
               const double *z, int64_t q, const int32_t *folds, int32_t nfolds,
               const int64_t *path, int64_t npath, int32_t rank, int32_t world,
               double *mses_raw);
/* The sharding rule of mih_cv_iht / mih_cv_mv (the reference's pmap / @threads hands combinations to workers as they come,
 * cross_validation.jl:98-121): rank_of[fold * npath + ik] = the rank of `world` that evaluates combination (fold, path[ik]).
 * Combinations are dealt out round-robin in the order (k descending, fold ascending), so every rank gets a stratified sample
 * of the model sizes (a fit's iteration count depends mostly on k).  No device needed. */
int mih_cv_assignment(const int64_t *path, int64_t npath, int32_t nfolds, int32_t world, int32_t *rank_of);
int mih_cv_meanloss(const double *mses_raw, const int32_t *folds, int64_t n, int32_t nfolds,
                    int64_t npath, double *mse_out);
/* iht_run_many_models(y, x, z; path, ...) src/cross_validation.jl:232-273: fit_iht on the FULL data for every
 * model size in path (no hold-out).  The fits advance in lock-step like the cross-validation fits (one fused
 * multi-RHS X'r pass per round), est_r included (every fit starts from prm->nb_r, as each fit_iht call of the reference builds
 * its own IHTVariable, :254-258).  Entry i is fitted by rank mih_cv_assignment(path, npath, 1, world)[i] (largest models first,
 * round-robin); logl_out[npath] (others 0), and optionally iter_out[npath], beta_out[npath*p], c_out[npath*q] (may be NULL). */
int mih_fit_iht_path(const mih_mat *h, const mih_fit_params *prm, const double *y, const double *z,
                     int64_t q, const int64_t *path, int64_t npath, int32_t rank, int32_t world,
                     double *logl_out, int64_t *iter_out, double *beta_out, double *c_out);
/* The same cross-validation driven from ONE process over several GPUs, the way the reference drives it
 * from several threads of one Julia process (Threads.@threads over the (fold,k) combinations on a shared x,
 * cross_validation.jl:100-112): hs[g] is a replica of the matrix on GPU g (they may also share a device),
 * one host thread per replica runs mih_cv_iht(hs[g], ..., rank = g, world = nrep) -- the combinations mih_cv_assignment gives
 * to g, or with est_r the chains c with c mod nrep == g -- and mses_raw receives the complete nfolds x npath matrix (no
 * separate reduction step). */
int mih_cv_iht_multi(const mih_mat *const *hs, int32_t nrep, const mih_fit_params *prm, const double *y,
                     const double *z, int64_t q, const int32_t *folds, int32_t nfolds,
                     const int64_t *path, int64_t npath, double *mses_raw);

/* ---- multivariate Gaussian IHT (src/multivariate.jl) ------------------------ */
typedef struct mih_mv_result {
    double   time, logl;
    int64_t  iter;
    int32_t  choose_fired, n_trace;
    double  *B;               /* r x p */
    double  *C;               /* r x q */
    double  *Sigma;           /* r x r = inv(Gamma) */
    double  *pve;             /* r */
    double  *logl_trace, *tol_trace;
    int32_t *bt_trace;
} mih_mv_result;
/* fit_iht(Y, Transpose(x), Z; d=MvNormal) : Y r x n, Z q x n column-major.
 * prm->comm != NULL: this process's shard of a column-sharded multivariate fit (round 5) -- h and B (r x local p) cover the local
 * columns, Y, Z, C, Sigma, the traces are replicated; per iteration one all-reduce of n r + 1 doubles (X_S df_S of iht_stepsize!,
 * multivariate.jl:220-254), one of n r doubles per update_xb! (:21-31) and one all-gather of 1 + 2K doubles per project_k! (the
 * shards' top-K entries of vec(B) as (global linear index, value) pairs).  init_beta and more than K exact ties at one shard's
 * threshold are refused. */
int mih_fit_mv(const mih_mat *h, const mih_fit_params *prm, const double *Y, int64_t r,
               const double *Z, int64_t q, const uint8_t *train, mih_mv_result *res);
int mih_cv_mv(const mih_mat *h, const mih_fit_params *prm, const double *Y, int64_t r,
              const double *Z, int64_t q, const int32_t *folds, int32_t nfolds,
              const int64_t *path, int64_t npath, int32_t rank, int32_t world, double *mses_raw);

/* ---- stepping session: one IHTVariable kept alive across calls ---------------- */
/* `initialize(...)` (src/data_structures.jl:117-135) + repeated `iht_one_step!`
 * (src/fit.jl:213-263) under the caller's control; used by bench.py to time exactly K
 * iterations and by callers that want their own convergence logic. */
typedef struct mih_session mih_session;
int mih_session_create(const mih_mat *h, const mih_fit_params *prm, const double *y,
                       const double *z, int64_t q, const uint8_t *train, mih_session **out);
/* save_prev! + iht_one_step! + check_convergence (fit.jl:182-193) */
int mih_session_step(mih_session *s, double *logl, int32_t *backtracks, double *tol);
/* `nsteps` such steps in one call -- the loop of fit_iht! (fit.jl:182-205) without its convergence test; logl and tol are
 * those of the last step, *backtracks the total */
int mih_session_run(mih_session *s, int64_t nsteps, double *logl, int64_t *backtracks, double *tol);
/* current model (v.b, v.c), not the best-so-far copy */
int mih_session_model(mih_session *s, double *beta, double *c);
int mih_session_destroy(mih_session *s);

/* ---- measurement hooks (bench.py; no reference counterpart) ----------------- */
/* The hook hangs on the matrix handle (no process-wide state).  While enabled, every launch of the dominant X'r kernel on
 * this matrix is bracketed by HIP events on the stream it is launched on and recorded with the name of the kernel that was
 * dispatched and the number of residuals it scored; the lock-step drivers (cv_iht, model paths) count what they did. */
typedef struct mih_pass_record {
    double  start_ms;         /* kernel start, relative to the mih_profile_enable(h, 1) call */
    double  ms;               /* kernel duration (HIP events on its own stream) */
    int32_t residuals;        /* residual vectors scored by this launch */
    int32_t operands;         /* B operands of the launch (32 digit columns each; a residual takes 10 in the default format) */
    int32_t stream_tag;       /* 0 = the handle's / a single fit's stream; 1, 2 = lock-step lanes */
    int32_t reserved;
    char    kernel[48];       /* e.g. "k_xtv_dma<1,2,4,8,fp4>" or "k_xtv_dma16<5,2,8,4,half>" */
} mih_pass_record;
enum { MIH_CNT_LANES = 0,          /* lock-step lanes started (summed over calls) */
       MIH_CNT_MAX_IN_FLIGHT = 1,  /* most fits in flight at once over all lanes */
       MIH_CNT_HANDOVERS = 2,      /* tail hand-overs (lane 1's fits adopted by lane 0) */
       MIH_CNT_SHARED_INIT = 3,    /* fits that started from another fit's initial score */
       MIH_CNT_ROUNDS = 4,         /* lock-step rounds */
       MIH_CNT_FITS = 5,           /* fits completed by the lock-step drivers */
       MIH_CNT_SCORES = 6,         /* IHT iterations of those fits as fit.jl counts them (one score ends each -- except a fit's last, see [14]) */
       MIH_CNT_MAX_LANE_SLOTS = 7, /* most fits in flight on ONE lane */
       MIH_CNT_INIT_SCORES = 8,    /* initial scores (init_iht_indices!, one per fit): rode a pass or were served by a copy */
       MIH_CNT_RESIDENT_STEPS = 9, /* iht_one_step! calls that ran resident on the device (step_mode 0; single fits, sessions and -- round 6 -- the lock-step drivers' fits) */
       MIH_CNT_RESIDENT_ATTEMPTS = 10, /* series of attempt slots that ended with their step still backtracking (it went on in the next series) */
       MIH_CNT_RESIDENT_HANDBACKS = 11, /* steps the device handed back to the host-driven path (_choose! ties, lists beyond its buffers) */
       MIH_CNT_RESIDENT_DIRECT = 12, /* attempts whose projection was queued as a direct gather (threshold forecast, verified) */
       MIH_CNT_RESIDENT_REDOS = 13,  /* ... of which the forecast failed: re-queued with the two histogram sweeps */
       MIH_CNT_SKIPPED_LAST_SCORES = 14, /* lock-step fits that converged: their last step's score (which the reference computes and never reads) was not computed */
       MIH_CNT_RESIDUALS_43BIT = 15, /* xtv_digits = -1: residuals the lock-step drivers scored in the 43-bit format (the rest: 54-bit) */
       MIH_CNT_PEELED_RESIDUALS = 16, /* residuals whose outlier guard fired: up to 64 rows towering over the rest left the fixed point and
                                       * rode the f64 side channel of k_xtv_finalize (csrc/peel.h); counted by mih_xtv_batched_fmt, mih_fit_iht, mih_fit_mv
                                       * and the lock-step drivers when they end */
       MIH_PROFILE_NCOUNTERS = 17 };
int mih_profile_enable(const mih_mat *h, int on);
/* synchronises the recorded launches; totals since the last reset */
int mih_profile_read(const mih_mat *h, double *xtv_kernel_ms, int64_t *xtv_launches, int reset);
/* the launches themselves, oldest first: up to cap records into out (may be NULL to ask for the count), *n = available */
int mih_profile_passes(const mih_mat *h, mih_pass_record *out, int64_t cap, int64_t *n, int reset);
/* exchanges of the column-sharded fits run on h while the hook was on, by kind: [0] all-reduce of n + 1 doubles (X_S g_S of
 * iht_stepsize! with the shards' |df_S|^2 riding along), [1] all-reduce of n doubles (X_S b_S of update_xb!), [2] all-gather of the
 * projection's candidates, [3] scalar exchanges on the host.  ms4 = summed duration (HIP events on the fit's stream for the
 * collectives queued there, the host clock for those the host waits for), count4 = how many. */
int mih_profile_exchange(const mih_mat *h, double *ms4, int64_t *count4, int reset);
int mih_profile_counters(const mih_mat *h, int64_t *out /* [MIH_PROFILE_NCOUNTERS] */, int reset);
/* Runs `iters` X'r passes of m residuals back to back on the handle's stream with R resident in HBM, bracketed by HIP
 * events; *ms_per_pass = average time of the whole chain (statistics, digit planes, pass, finalize).  m = 1 uses the
 * workspace of a single univariate fit, m > 1 the fused multi-residual one; digits as in mih_xtv_batched_fmt. */
int mih_bench_xtv(const mih_mat *h, int digits, int m, int iters, int warmup, uint64_t seed,
                  float *ms_per_pass, double *checksum);
/* Algorithmic bytes of one X'r pass: p*ceil(n/4) + 8*m*(n+p) + 16*p. */
int mih_xtv_algorithmic_bytes(const mih_mat *h, int m, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* MENDELIHT_HIP_H */
