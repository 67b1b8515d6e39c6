// variants_pca_driver.cpp -- compiled host of the PCoA engine: the VariantsPcaDriver command line
// (reference src/main/scala/com/google/cloud/genomics/spark/examples/VariantsPca.scala:36-52 and
// GenomicsConf.scala:31-101) over the C ABI of include/pcoa.h.  No Python, no torch, no Spark.
//
//   main (:38-50)            conf -> data -> filterDataset -> getCallsRdd -> getSimilarityMatrix ->
//                            computePca -> emitResult -> reportIoStats -> stop
//   getVariantKey (:62-78)   Guava murmur3_128 over contig, start, end, ref, alt
//   filterDataset (:96-108)  --min-allele-frequency on INFO/AF
//   joinDatasets (:115-128)  two variant sets: inner join on the key
//   mergeDatasets (:136-148) three or more: group by key, keep complete groups
//   getCallsRdd (:153-168)   carriers per variant; variants without a varying call dropped
//   emitResult (:233-246)    name \t dataset \t pc1 \t pc2 sorted by name (+ <output-path>-pca.tsv)
//
// The data source is local: one VCF (plain or .gz via a spawned `gzip -dc`) per variant set -- the Google
// Genomics API the reference streamed from (VariantsRDD.scala) has been shut down.  Callset index =
// position in the concatenated sample lists (VariantsCommon.scala:44-45), callset id =
// "<file stem>-<i>", so `dataset` = id up to the first '-' (:235) is the file stem.
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>
#include <chrono>
#include <set>

#include <spawn.h>
#include <sys/wait.h>
#include <unistd.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <functional>
#include <future>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <sys/resource.h>

extern char** environ;

#include "pcoa.h"

namespace {

struct Conf {  // PcaConf / GenomicsConf (GenomicsConf.scala:31-101), same flag names and defaults
  std::vector<std::string> input_path;
  std::string output_path;
  std::vector<std::string> references{"chr17:41196311:41277499"};
  std::vector<std::string> variant_set_id{"3049512673186936334"};
  bool all_references = false, debug_datasets = false, has_maf = false;
  bool parse_only = false;  // not a reference flag: ingest + getCallsRdd only, prints the carrier statistics (no GPU)
  std::string dump_similarity;  // not a reference flag: writes S (N x N int64, little-endian, row-major) for parity tests
  int ingest_threads = 0;   // not a reference flag: 0 = hardware concurrency (local[*]), cf. --spark-master local[k]
  std::string plink_ref_allele = "a2";  // not a reference flag: which .bim allele column is REF (a2 = --keep-allele-order)
  float min_allele_frequency = 0.f;
  int num_pc = 2, num_reduce_partitions = 10, gpu = 0;
  long bases_per_partition = 1000000;
  std::string client_secrets, spark_master;
  // r04: the variant-sharded job of BASELINE configs[2] from the command line (VariantsPca.scala:190: partitions + reduceByKey)
  int gpus = 1;                       // --gpus k: k host threads, one engine per device, variants dealt by contiguous ranges
  std::vector<int> gpu_map;           // --gpu-map a,b,..: device ordinal of each engine (default: --gpu, --gpu + 1, ..)
  std::string reduce = "auto";        // --reduce auto|rccl|peer|scatter: all-reduce over RCCL / peer copies + adds into engine 0, one
                                      // engine after the other / reduce-scatter over all k engines at once (pcoa_gram_reduce_peers)
  std::string layout = "auto";        // --layout auto|full|strips: S whole on every engine (variants dealt, then reduced) or
                                      // tiled by columns (every engine fed every variant, no reduction); auto: pcoa_plan_layout
  std::string plink_decode = "device";  // --plink-decode device|host: where the 2-bit codes become carrier bits
  long stream_rows = 131072;          // --stream-rows: variants per block of the streaming PLINK reader (four blocks are page-locked: 328 MB at N = 2504)
  bool no_stream = false;             // --no-stream: a single PLINK fileset / VCF through the in-memory path (whole data set, then carrier lists)
  int join_partitions = 64;             // --join-partitions P (r06): joins / merges of several VCFs are hash-partitioned on getVariantKey into P spill
                                        // files per variant set; one partition (1 / P of every set) is in memory at a time
  std::string spill_dir;                // --spill-dir: where those files go (default $TMPDIR, else /tmp)
  bool spark_output = false;            // --spark-output-layout (r06): <output-path>-pca.tsv as the DIRECTORY saveAsTextFile leaves (part-00000 + _SUCCESS,
                                        // VariantsPca.scala:241-245) instead of one file of that name
  std::string carrier_format = "auto";  // --carrier-format auto|lists|bits (r06): how RDD[Seq[Int]] rows cross to the engine -- auto: a block
                                        // whose mean list is longer than N / 32 entries goes over as carrier bitsets (fewer bytes), else as lists
  std::vector<std::string> project_input_path;  // --project-input-path: VCFs whose samples are placed onto the PCA of --input-path
                                                // (pcoa_project); their callsets follow the reference's, variants matched by join / merge
  std::string gram = "stored";          // --gram stored|implicit: stored = S is accumulated and decomposed (every path above); implicit = one
                                        // operator engine (pcoa_create_operator) keeps the carrier bitsets and computePca runs over the
                                        // products S v = X^T (X v): no N x N matrix exists.  No auto: which form is faster at which N
                                        // has not been measured
  bool grm = false;                     // --grm: standardised-genotype PCA: one GRM engine (pcoa_create_grm) keeps the 2-bit genotypes of ONE
                                        // streamed PLINK fileset and computePca decomposes K = Z^T Z / M (the matrix of smartpca, plink --pca,
                                        // GCTA, flashpca) through the products K x: no N x N matrix exists
  double grm_min_maf = 0.0;             // --grm-min-maf X: --grm uses only variants whose minor-allele frequency is at least X, in [0, 0.5)
  bool has_grm_min_maf = false;
  double grm_geno = 1.0;                // --grm-geno X: --grm uses only variants whose share of missing calls is at most X, in [0, 1] (plink --geno)
  double grm_hwe = 0.0;                 // --grm-hwe P: ... and whose Hardy-Weinberg exact-test p-value is at least P, in [0, 1) (plink --hwe)
  double grm_mind = 1.0;                // --grm-mind X: samples whose share of missing calls exceeds X are taken out before anything else (plink --mind)
  bool has_grm_geno = false, has_grm_hwe = false, has_grm_mind = false;
  std::string grm_variant_qc_output_path;   // --grm-variant-qc-output-path FILE: index, contig, position, id, n, het, hom-alt, missing share, HWE p, used
  std::string grm_sample_qc_output_path;    // --grm-sample-qc-output-path FILE: name, called, het, hom-alt, call rate, het share of called, kept
  std::string grm_output_path;          // --grm-output-path PREFIX: --grm: K read out band by band into PREFIX.grm.bin / .grm.N.bin / .grm.id
  std::string grm_output_divisor;       // --grm-output-divisor used|pairwise: num / M' (default) or num / n(i, j)
  bool has_grm_output_divisor = false;
  std::string grm_weights_output_path;  // --grm-weights-output-path FILE: --grm: the SNP weight of every variant on each of the --num-pc axes of K
  std::string grm_project_path;         // --grm-project-path STUDY.bed: --grm: a second PLINK fileset whose samples are placed onto the panel's axes
  std::string grm_keep_samples;         // --grm-keep-samples FILE: --grm: one sample name per line; the PCA runs on the engine's subset over these samples
  std::string grm_remove_samples;       // --grm-remove-samples FILE: the same, the file names the samples that are taken out
  int grm_outlier_iterations = 0;       // --grm-outlier-iterations K: --grm: the rounds of --outlier-iterations with the engine replaced by its
                                        // pcoa_create_grm_subset over the kept samples
  double grm_outlier_sigma = 6.0;       // --grm-outlier-sigma X: their threshold
  bool grm_outlier_sigma_given = false;
  bool grm_cutoff_given = false;        // --grm-cutoff X given: --grm: the relatedness screen of K before computePca (pcoa_grm_pairs): a pair is
  double grm_cutoff = 0.0;              // reported when K(i, j) >= X
  std::string grm_cutoff_text;          // X as it was typed (for the refusal of a value that is not a finite number)
  std::string grm_cutoff_divisor;       // --grm-cutoff-divisor used|pairwise: the K that is screened: num / M' (default) or num / n(i, j)
  bool has_grm_cutoff_divisor = false;
  std::string grm_related_output_path;  // --grm-related-output-path FILE: the reported pairs, one line each
  bool has_grm_related_output_path = false;
  bool grm_king = false;                // --grm-king-cutoff X given: --grm: the KING-robust kinship screen of the genotype store before computePca
  double grm_king_cutoff = 0.0;         // (pcoa_grm_king_pairs), where --grm-cutoff runs: a pair is reported when (hethet - 2 ibs0) / het_sum >= X
  std::string grm_king_rows;            // --grm-king-rows all|used: the counted variants: used_v (default) or every row of the store
  bool has_grm_king_rows = false;
  std::string grm_king_output_path;     // --grm-king-output-path FILE: the reported pairs in the format of --king-output-path
  bool has_grm_king_output_path = false;
  int64_t grm_king_max_pairs = 1048576; // --grm-king-max-pairs M: the capacity handed to the library; more reported pairs stop the job
  bool grm_king_max_pairs_given = false;
  std::string grm_pcrelate_output_path;             // --grm-pcrelate-output-path FILE: --grm: PC-Relate kinship (pcoa_grm_pcrelate_*) behind the last
  bool has_grm_pcrelate_output_path = false;        // computePca and --grm-project-removed; the pairs at or above the cutoff go to FILE
  int grm_pcrelate_pcs = 0;                         // --grm-pcrelate-pcs K: the axes beside the intercept, [1, min(8, --num-pc)]; default min(2, --num-pc)
  bool has_grm_pcrelate_pcs = false;
  double grm_pcrelate_cutoff = 0.044194173824159216;   // --grm-pcrelate-cutoff X: 2^-4.5
  bool has_grm_pcrelate_cutoff = false;
  double grm_pcrelate_maf_threshold = 0.01;         // --grm-pcrelate-maf-threshold T in [0, 0.5)
  bool has_grm_pcrelate_maf_threshold = false;
  std::string grm_pcrelate_inbreeding_output_path;  // --grm-pcrelate-inbreeding-output-path FILE: name, f = 2 phi(i, i) - 1, n(i, i)
  bool has_grm_pcrelate_inbreeding_output_path = false;
  int64_t grm_pcrelate_max_pairs = 1048576;         // --grm-pcrelate-max-pairs M: the capacity handed to the library; more reported pairs stop the job
  bool grm_pcrelate_max_pairs_given = false;
  bool grm_king_remove = false;         // --grm-king-remove: drop one sample of every reported pair, go on with pcoa_create_grm_subset over the rest
  bool grm_cutoff_remove = false;       // --grm-cutoff-remove: drop one sample of every reported pair, go on with pcoa_create_grm_subset over the rest
  bool grm_project_lsq = false;         // --grm-project-lsq: both projections place by least squares over the called variants (pcoa_grm_project_lsq)
  bool grm_project_removed = false;     // --grm-project-removed: the samples a list or a round removed are placed on the final axes
  int outlier_iterations = 0;           // --outlier-iterations K: up to K rounds of outlier removal around computePca; a round replaces the engine by
                                        // its subset over the kept samples (pcoa_create_subset: one gather of S, no variant read twice).  0 = off
  double outlier_sigma = 6.0;           // --outlier-sigma X: a sample further than X population standard deviations from the mean of an axis goes
  bool related = false;                 // --related-min-jaccard X given: screen S for duplicate and related sample pairs before computePca
  double related_min_jaccard = 0.0;     // (pcoa_similar_pairs): a pair is reported when S(i, j) >= X (S(i, i) + S(j, j) - S(i, j)); X in (0, 1]
  std::string related_output_path;      // --related-output-path FILE: the reported pairs, one line each
  int64_t related_max_pairs = 1048576;  // --related-max-pairs M: the capacity handed to the library; more reported pairs stop the job
  bool related_max_pairs_given = false;
  bool remove_related = false;          // --remove-related: drop one sample of every reported pair, go on with pcoa_create_subset over the rest
  bool king = false;                    // --king-cutoff X given: the KING-robust kinship screen before computePca (pcoa_king_pairs) over five
  double king_cutoff = 0.0;             // plane engines fed the same streamed .bed blocks (pcoa_accumulate_plink_bed_king); X in (0, 0.5]
  std::string king_output_path;         // --king-output-path FILE: the reported pairs, one line each
  int64_t king_max_pairs = 1048576;     // --king-max-pairs M: the capacity handed to the library; more reported pairs stop the job
  bool king_max_pairs_given = false;
  bool king_remove = false;             // --king-remove: the rule of --remove-related over the pairs of the kinship screen
  std::string similarity_measure = "shared";  // --similarity-measure shared|jaccard|cosine: what computePca decomposes (pcoa_set_similarity);
                                              // jaccard / cosine are evaluated on the fly from S, set on the engine that runs computePca
  std::string loadings_output_path;     // --loadings-output-path FILE: the loading of every variant fed to the engine on each of the --num-pc
                                        // principal coordinates, w_c = X (J u_c) / sqrt(lambda_c) (pcoa_loadings_*), one line per variant in feed
                                        // order.  --gram implicit reads the resident store; a stored S takes a second streaming pass over a
                                        // single PLINK fileset
  int grm_ld_window = 0;                // --grm-ld-window W: --grm: LD-prune the resident store by dosage r^2 (pcoa_grm_ld_prune), W store rows; 0 = off
  double grm_ld_r2 = 0.2;               // --grm-ld-r2 X: its threshold (the default of --ld-r2)
  bool grm_ld_r2_given = false;
  std::string grm_ld_output_path;       // --grm-ld-output-path FILE: one line per variant of the store: index, contig, position, id, 1 (kept) or 0
  int ld_window = 0;                    // --ld-window W: LD pruning in front of the accumulation (pcoa_ld_*), W fed variants; 0 = off
  double ld_r2 = 0.2;                   // --ld-r2 X: a variant is removed when a kept one inside the window has r^2 of the carrier indicators above X
  bool ld_r2_given = false;
  std::string ld_output_path;           // --ld-output-path FILE: one line per fed variant in feed order: index, contig, position, id, 1 (kept) or 0
  std::string missing_calls = "ignore";  // --missing-calls ignore|pairwise: pairwise decomposes S(i, j) / M(i, j), M the variants at which both
                                         // samples were called (pcoa_set_call_companion); a second engine, the companion, takes the
                                         // missing-call bitsets of the same streamed .bed blocks (pcoa_accumulate_plink_bed_calls)
  std::string call_rate_output_path;     // --call-rate-output-path FILE: name, called variants, variants fed, call rate per sample
  int32_t similarity_kind() const {
    return similarity_measure == "jaccard" ? PCOA_SIMILARITY_JACCARD : similarity_measure == "cosine" ? PCOA_SIMILARITY_COSINE : PCOA_SIMILARITY_SHARED;
  }
};

const char* kUsage =
    "usage: variants_pca_driver --input-path <file.vcf[.gz]> [more] | <prefix>.bed [options]\n"
    "  reference flags: --output-path P --num-pc K --references R.. --all-references --min-allele-frequency F\n"
    "                   --debug-datasets --bases-per-partition B --num-reduce-partitions P --variant-set-id ..\n"
    "  engine flags:    --gpu D --gpus K --gpu-map a,b,.. --reduce auto|rccl|peer|scatter --layout auto|full|strips\n"
    "                   --gram stored|implicit --carrier-format auto|lists|bits --plink-decode device|host\n"
    "                   --plink-ref-allele a1|a2 --stream-rows R\n"
    "                   --no-stream --join-partitions P --spill-dir D --spark-output-layout --ingest-threads T\n"
    "                   --parse-only --dump-similarity FILE\n"
    "                   --outlier-iterations K --outlier-sigma X (K rounds: samples beyond X sd on a principal component are\n"
    "                   removed and computePca runs again on S[kept, kept]; one engine, stored S, full layout)\n"
    "                   --related-min-jaccard X [--related-output-path FILE] [--related-max-pairs M] [--remove-related]\n"
    "                   (before computePca: report the sample pairs whose carrier sets have a Jaccard index >= X, X in (0, 1];\n"
    "                   --remove-related drops one sample of each pair and decomposes S[kept, kept]; one engine, stored S,\n"
    "                   full layout)\n"
    "                   --king-cutoff X [--king-output-path FILE] [--king-max-pairs M] [--king-remove]\n"
    "                   (before computePca: report the sample pairs whose KING-robust kinship (hethet - 2 ibs0) / het_sum is >= X,\n"
    "                   X in (0, 0.5], 0.177 = first degree; independent of allele frequencies; --king-remove drops one sample of\n"
    "                   each pair as --remove-related does; one streamed PLINK fileset, one device, five more N x N matrices)\n"
    "                   --grm [--grm-min-maf X] (standardised-genotype PCA: decompose K = Z^T Z / M over allele-frequency-standardised\n"
    "                   dosages, missing calls mean-imputed -- the matrix of smartpca, plink --pca, GCTA, flashpca -- through the\n"
    "                   products K x of one GRM engine that keeps 2 bits per genotype; X in [0, 0.5); one streamed PLINK fileset,\n"
    "                   one device, no N x N matrix)\n"
    "                   --grm-weights-output-path FILE (--grm: the SNP weight of every variant on each of the --num-pc axes of K, in the\n"
    "                   format of --loadings-output-path; an unused variant prints 0.0)\n"
    "                   --grm-project-path STUDY.bed (--grm: a second PLINK fileset whose samples are placed onto the panel's axes\n"
    "                   without moving them; its .bim must equal the panel's line by line; its rows follow the panel's)\n"
    "                   --grm-output-path PREFIX [--grm-output-divisor used|pairwise] (--grm: the matrix that was decomposed, read out\n"
    "                   band by band: PREFIX.grm.bin (float32 lower triangle with the diagonal), PREFIX.grm.N.bin (jointly called used\n"
    "                   variants per pair) and PREFIX.grm.id, the layout GCTA and PLINK read; used: num / M', pairwise: num / n(i, j))\n"
    "                   --grm-keep-samples FILE | --grm-remove-samples FILE (--grm: one sample name per line; the PCA runs on the engine's\n"
    "                   subset over the kept samples, one gather of the 2-bit store, with their own allele frequencies)\n"
    "                   --grm-outlier-iterations K [--grm-outlier-sigma X, default 6] (--grm: the rounds of --outlier-iterations on subsets\n"
    "                   of the genotype store; --grm-ld-window prunes every round's engine again)\n"
    "                   --grm-project-removed (--grm: the samples a list or a round removed are placed on the final axes)\n"
    "                   --grm-project-lsq (--grm-project-path / --grm-project-removed: place every sample by least squares over the used\n"
    "                   variants it is called at, not by mean imputation, which shrinks a sparsely called sample towards the origin;\n"
    "                   --grm-project-removed then places the samples --grm-mind took out too; at most 16 principal components)\n"
    "                   --grm-king-cutoff X [--grm-king-rows all|used] [--grm-king-output-path FILE] [--grm-king-max-pairs M] [--grm-king-remove]\n"
    "                   (the KING-robust kinship screen of the genotype store, where --grm-cutoff runs: pcoa_grm_king_pairs)\n"
    "                   --grm-pcrelate-output-path FILE [--grm-pcrelate-pcs K] [--grm-pcrelate-cutoff X] [--grm-pcrelate-maf-threshold T]\n"
    "                   [--grm-pcrelate-inbreeding-output-path FILE] [--grm-pcrelate-max-pairs M]\n"
    "                   (PC-Relate kinship over the final cohort and the placed removed samples, behind the last computePca: pcoa_grm_pcrelate_*)\n"
    "                   --grm-cutoff X [--grm-cutoff-divisor used|pairwise] [--grm-related-output-path FILE] [--grm-cutoff-remove]\n"
    "                   (--grm: screen K for related pairs before computePca, behind the sample list and one LD prune: a pair is reported\n"
    "                   when K(i, j) >= X; FILE: name_i, name_j, K, n per pair; --grm-cutoff-remove drops one sample of every pair by the\n"
    "                   rule of --remove-related and goes on with the engine's subset over the rest)\n"
    "                   --grm-ld-window W [--grm-ld-r2 X, default 0.2] [--grm-ld-output-path FILE] (--grm: LD-prune the resident store\n"
    "                   before computePca: forward and greedy, a used variant is removed when a kept one among the W rows before it\n"
    "                   on the same contig has r^2 of the dosages over the jointly called samples above X -- plink's pair statistic,\n"
    "                   the earlier kept variant wins; FILE: index, contig, position, id, 1 (kept) or 0 per variant)\n"
    "                   --grm-geno X, --grm-hwe P, --grm-mind X (--grm: the quality filters of plink: a variant is used only when its share\n"
    "                   of missing calls is at most X and its Hardy-Weinberg exact-test p-value (no mid-p) at least P; samples whose\n"
    "                   share of missing calls exceeds --grm-mind are taken out first and are not placed by --grm-project-removed)\n"
    "                   --grm-variant-qc-output-path FILE (--grm: index, contig, position, id, called, het, hom-alt, missing share, HWE p,\n"
    "                   1 (used) or 0 per variant) --grm-sample-qc-output-path FILE (name, called, het, hom-alt, call rate, het share\n"
    "                   of called, 1 (kept) or 0 per sample)\n"
    "                   --similarity-measure shared|jaccard|cosine (what computePca decomposes: the counts S as the reference,\n"
    "                   S(i,j) / (S(i,i) + S(j,j) - S(i,j)), or S(i,j) / sqrt(S(i,i) S(j,j)), evaluated on the fly from S; one\n"
    "                   engine, stored S, full layout, no projection)\n"
    "                   --loadings-output-path FILE (the loading of every variant on each of the --num-pc principal coordinates,\n"
    "                   one line per variant in feed order: index, contig, position, id, loadings; one engine, the whole\n"
    "                   cohort, --similarity-measure shared; --gram implicit for any input, a stored S for one streamed PLINK\n"
    "                   fileset)\n"
    "                   --ld-window W [--ld-r2 X, default 0.2] [--ld-output-path FILE] (LD pruning on the device in front of the\n"
    "                   accumulation: forward and greedy in feed order, a variant is removed when it is monomorphic or when a KEPT\n"
    "                   variant among the W fed before it, on the same contig, has r^2 of the carrier indicators above X; FILE gets\n"
    "                   one line per fed variant: index, contig, position, id, 1 or 0; one engine, one input set)\n"
    "                   --missing-calls ignore|pairwise [--call-rate-output-path FILE] (pairwise: computePca decomposes\n"
    "                   S(i,j) / M(i,j), M the variants at which both samples were called, evaluated on the fly from S and the\n"
    "                   Gram matrix of the missing calls; FILE gets one line per sample: name, called variants, variants fed,\n"
    "                   call rate; one streamed PLINK fileset, one engine, stored S, full layout, --similarity-measure shared, no\n"
    "                   projection, loadings or LD pruning)\n"
    "  --project-input-path <file.vcf[.gz]> [more]\n"
    "                   place these samples onto the principal coordinates of the --input-path cohort instead of\n"
    "                   decomposing the union (one GPU, VCF inputs, full layout)\n";

[[noreturn]] void die(const std::string& m) {
  std::cerr << "VariantsPcaDriver: " << m << std::endl;
  std::exit(2);
}

const char* kStripsRefuseOutliers = "--outlier-iterations subsets one whole similarity matrix on one engine: it cannot take --layout strips";
std::string strips_refuse_measure(const std::string& m) {
  return "--similarity-measure " + m + " needs the diagonal of one whole similarity matrix on one engine: it cannot take --layout strips";
}
const char* kStripsRefuseMissing = "--missing-calls pairwise needs two whole similarity matrices on one device: it cannot take --layout strips";
const char* kStripsRefuseRelated = "--related-min-jaccard screens one whole similarity matrix on one engine: it cannot take --layout strips";
const char* kStripsRefuseKing = "--king-cutoff screens five whole Gram matrices on one device: it cannot take --layout strips";

Conf parse(int argc, char** argv) {
  Conf c;
  auto list = [&](int& i, std::vector<std::string>& dst) {
    dst.clear();
    while (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) dst.push_back(argv[++i]);
  };
  auto one = [&](int& i) -> std::string {
    if (i + 1 >= argc) die(std::string("missing value for ") + argv[i]);
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--input-path") list(i, c.input_path);
    else if (a == "--project-input-path") {
      list(i, c.project_input_path);
      if (c.project_input_path.empty()) die("--project-input-path needs at least one file");
    }
    else if (a == "--help" || a == "-h") { std::fputs(kUsage, stdout); std::exit(0); }
    else if (a == "--references") list(i, c.references);
    else if (a == "--variant-set-id") list(i, c.variant_set_id);
    else if (a == "--output-path") c.output_path = one(i);
    else if (a == "--num-pc") c.num_pc = std::atoi(one(i).c_str());
    else if (a == "--min-allele-frequency") { c.min_allele_frequency = std::strtof(one(i).c_str(), nullptr); c.has_maf = true; }
    else if (a == "--all-references") c.all_references = true;
    else if (a == "--debug-datasets") c.debug_datasets = true;
    else if (a == "--bases-per-partition") c.bases_per_partition = std::atol(one(i).c_str());
    else if (a == "--num-reduce-partitions") c.num_reduce_partitions = std::atoi(one(i).c_str());
    else if (a == "--client-secrets") c.client_secrets = one(i);
    else if (a == "--spark-master") c.spark_master = one(i);
    else if (a == "--gpu") c.gpu = std::atoi(one(i).c_str());
    else if (a == "--gpus") c.gpus = std::atoi(one(i).c_str());
    else if (a == "--gpu-map") {
      std::stringstream ss(one(i));
      std::string tok;
      c.gpu_map.clear();
      while (std::getline(ss, tok, ',')) c.gpu_map.push_back(std::atoi(tok.c_str()));
    }
    else if (a == "--reduce") c.reduce = one(i);
    else if (a == "--layout") c.layout = one(i);
    else if (a == "--plink-decode") c.plink_decode = one(i);
    else if (a == "--stream-rows") c.stream_rows = std::atol(one(i).c_str());
    else if (a == "--no-stream") c.no_stream = true;
    else if (a == "--spark-output-layout") c.spark_output = true;
    else if (a == "--join-partitions") { c.join_partitions = std::atoi(one(i).c_str()); if (c.join_partitions < 1) die("--join-partitions must be >= 1"); }
    else if (a == "--spill-dir") c.spill_dir = one(i);
    else if (a == "--carrier-format") {
      c.carrier_format = one(i);
      if (c.carrier_format != "auto" && c.carrier_format != "lists" && c.carrier_format != "bits") die("--carrier-format takes auto, lists or bits");
    }
    else if (a == "--gram") {
      c.gram = one(i);
      if (c.gram != "stored" && c.gram != "implicit") die("--gram takes stored or implicit");
    }
    else if (a == "--grm") c.grm = true;
    else if (a == "--grm-weights-output-path") c.grm_weights_output_path = one(i);
    else if (a == "--grm-project-path") c.grm_project_path = one(i);
    else if (a == "--grm-output-path") c.grm_output_path = one(i);
    else if (a == "--grm-output-divisor") {
      c.grm_output_divisor = one(i);
      c.has_grm_output_divisor = true;
    }
    else if (a == "--grm-min-maf") {
      const std::string v = one(i);
      char* end = nullptr;
      c.grm_min_maf = std::strtod(v.c_str(), &end);
      c.has_grm_min_maf = true;
      if (v.empty() || *end != 0 || !(c.grm_min_maf >= 0.0 && c.grm_min_maf < 0.5))
        die("--grm-min-maf takes a frequency in [0, 0.5), not '" + v + "'");
    }
    else if (a == "--grm-geno" || a == "--grm-hwe" || a == "--grm-mind") {
      const std::string v = one(i);
      char* end = nullptr;
      const double x = std::strtod(v.c_str(), &end);
      const bool parsed = !v.empty() && *end == 0;
      if (a == "--grm-hwe") {
        if (!parsed || !(x >= 0.0 && x < 1.0)) die("--grm-hwe takes a p-value in [0, 1), not '" + v + "'");
        c.grm_hwe = x;
        c.has_grm_hwe = true;
      } else {
        if (!parsed || !(x >= 0.0 && x <= 1.0)) die(a + " takes a share of missing calls in [0, 1], not '" + v + "'");
        (a == "--grm-geno" ? c.grm_geno : c.grm_mind) = x;
        (a == "--grm-geno" ? c.has_grm_geno : c.has_grm_mind) = true;
      }
    }
    else if (a == "--grm-variant-qc-output-path") c.grm_variant_qc_output_path = one(i);
    else if (a == "--grm-sample-qc-output-path") c.grm_sample_qc_output_path = one(i);
    else if (a == "--grm-keep-samples") c.grm_keep_samples = one(i);
    else if (a == "--grm-remove-samples") c.grm_remove_samples = one(i);
    else if (a == "--grm-project-removed") c.grm_project_removed = true;
    else if (a == "--grm-project-lsq") c.grm_project_lsq = true;
    else if (a == "--grm-cutoff") {
      c.grm_cutoff_text = one(i);
      char* end = nullptr;
      c.grm_cutoff = std::strtod(c.grm_cutoff_text.c_str(), &end);
      c.grm_cutoff_given = true;
      if (c.grm_cutoff_text.empty() || *end != 0) die("--grm-cutoff takes a number, not '" + c.grm_cutoff_text + "'");
    }
    else if (a == "--grm-cutoff-divisor") {
      c.grm_cutoff_divisor = one(i);
      c.has_grm_cutoff_divisor = true;
    }
    else if (a == "--grm-related-output-path") {
      c.grm_related_output_path = one(i);
      c.has_grm_related_output_path = true;
    }
    else if (a == "--grm-cutoff-remove") c.grm_cutoff_remove = true;
    else if (a == "--grm-king-cutoff") {
      const std::string v = one(i);
      char* end = nullptr;
      c.grm_king_cutoff = std::strtod(v.c_str(), &end);
      if (v.empty() || *end != 0) die("--grm-king-cutoff takes a number in (0, 0.5], not '" + v + "'");
      c.grm_king = true;
    }
    else if (a == "--grm-king-rows") {
      c.grm_king_rows = one(i);
      c.has_grm_king_rows = true;
    }
    else if (a == "--grm-king-output-path") {
      c.grm_king_output_path = one(i);
      c.has_grm_king_output_path = true;
    }
    else if (a == "--grm-king-max-pairs") {
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long long m = std::strtoll(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0) die("--grm-king-max-pairs takes an integer >= 0, not '" + v + "'");
      c.grm_king_max_pairs = (int64_t)m;
      c.grm_king_max_pairs_given = true;
    }
    else if (a == "--grm-king-remove") c.grm_king_remove = true;
    else if (a == "--grm-pcrelate-output-path") {
      c.grm_pcrelate_output_path = one(i);
      c.has_grm_pcrelate_output_path = true;
    }
    else if (a == "--grm-pcrelate-inbreeding-output-path") {
      c.grm_pcrelate_inbreeding_output_path = one(i);
      c.has_grm_pcrelate_inbreeding_output_path = true;
    }
    else if (a == "--grm-pcrelate-pcs" || a == "--grm-pcrelate-max-pairs") {
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long long m = std::strtoll(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0) die(a + " takes an integer, not '" + v + "'");
      if (a == "--grm-pcrelate-pcs") {
        c.grm_pcrelate_pcs = (int)std::max<long long>(std::min<long long>(m, 1 << 30), -(1 << 30));
        c.has_grm_pcrelate_pcs = true;
      } else {
        c.grm_pcrelate_max_pairs = (int64_t)m;
        c.grm_pcrelate_max_pairs_given = true;
      }
    }
    else if (a == "--grm-pcrelate-cutoff" || a == "--grm-pcrelate-maf-threshold") {
      const std::string v = one(i);
      char* end = nullptr;
      const double x = std::strtod(v.c_str(), &end);
      if (v.empty() || *end != 0) die(a + " takes a number, not '" + v + "'");
      if (a == "--grm-pcrelate-cutoff") {
        c.grm_pcrelate_cutoff = x;
        c.has_grm_pcrelate_cutoff = true;
      } else {
        c.grm_pcrelate_maf_threshold = x;
        c.has_grm_pcrelate_maf_threshold = true;
      }
    }
    else if (a == "--grm-outlier-iterations") {
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long k = std::strtol(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0 || k > 1000000 || k < -1000000) die("--grm-outlier-iterations takes an integer >= 0 (0 = off), not '" + v + "'");
      c.grm_outlier_iterations = (int)k;
    }
    else if (a == "--grm-outlier-sigma") {
      const std::string v = one(i);
      char* end = nullptr;
      c.grm_outlier_sigma = std::strtod(v.c_str(), &end);
      c.grm_outlier_sigma_given = true;
      if (v.empty() || *end != 0) die("--grm-outlier-sigma (the threshold of --grm-outlier-iterations) takes a number, not '" + v + "'");
    }
    else if (a == "--outlier-iterations") {   // a value that does not parse must not silently mean "off"
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long k = std::strtol(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0 || k > 1000000 || k < -1000000) die("--outlier-iterations takes an integer >= 0 (0 = off), not '" + v + "'");
      c.outlier_iterations = (int)k;
    }
    else if (a == "--outlier-sigma") {
      const std::string v = one(i);
      char* end = nullptr;
      c.outlier_sigma = std::strtod(v.c_str(), &end);
      if (v.empty() || *end != 0) die("--outlier-sigma (the threshold of --outlier-iterations) takes a number, not '" + v + "'");
    }
    else if (a == "--related-min-jaccard") {   // a value that does not parse must not silently mean "off"
      const std::string v = one(i);
      char* end = nullptr;
      c.related_min_jaccard = std::strtod(v.c_str(), &end);
      if (v.empty() || *end != 0) die("--related-min-jaccard takes a number in (0, 1], not '" + v + "'");
      c.related = true;
    }
    else if (a == "--related-output-path") c.related_output_path = one(i);
    else if (a == "--related-max-pairs") {
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long long m = std::strtoll(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0) die("--related-max-pairs takes an integer >= 0, not '" + v + "'");
      c.related_max_pairs = (int64_t)m;
      c.related_max_pairs_given = true;
    }
    else if (a == "--remove-related") c.remove_related = true;
    else if (a == "--king-cutoff") {   // a value that does not parse must not silently mean "off"
      const std::string v = one(i);
      char* end = nullptr;
      c.king_cutoff = std::strtod(v.c_str(), &end);
      if (v.empty() || *end != 0) die("--king-cutoff takes a number in (0, 0.5], not '" + v + "'");
      c.king = true;
    }
    else if (a == "--king-output-path") c.king_output_path = one(i);
    else if (a == "--king-max-pairs") {
      const std::string v = one(i);
      char* end = nullptr;
      errno = 0;
      const long long m = std::strtoll(v.c_str(), &end, 10);
      if (v.empty() || *end != 0 || errno != 0) die("--king-max-pairs takes an integer >= 0, not '" + v + "'");
      c.king_max_pairs = (int64_t)m;
      c.king_max_pairs_given = true;
    }
    else if (a == "--king-remove") c.king_remove = true;
    else if (a == "--similarity-measure") {
      c.similarity_measure = one(i);
      if (c.similarity_measure != "shared" && c.similarity_measure != "jaccard" && c.similarity_measure != "cosine")
        die("--similarity-measure takes shared, jaccard or cosine, not '" + c.similarity_measure + "'");
    }
    else if (a == "--missing-calls") {
      c.missing_calls = one(i);
      if (c.missing_calls != "ignore" && c.missing_calls != "pairwise")
        die("--missing-calls takes ignore or pairwise, not '" + c.missing_calls + "'");
    }
    else if (a == "--call-rate-output-path") c.call_rate_output_path = one(i);
    else if (a == "--loadings-output-path") c.loadings_output_path = one(i);
    else if (a == "--ld-window") {
      const std::string v = one(i);
      char* end = nullptr;
      const long w = std::strtol(v.c_str(), &end, 10);
      if (v.empty() || *end || w < 0 || w > PCOA_LD_MAX_WINDOW)
        die("--ld-window takes a number of variants in [1, " + std::to_string(PCOA_LD_MAX_WINDOW) + "] (0: off), not '" + v + "'");
      c.ld_window = (int)w;
    }
    else if (a == "--ld-r2") {
      const std::string v = one(i);
      char* end = nullptr;
      c.ld_r2 = std::strtod(v.c_str(), &end);
      if (v.empty() || *end || !(c.ld_r2 >= 0.0 && c.ld_r2 <= 1.0)) die("--ld-r2 takes a threshold in [0, 1], not '" + v + "'");
      c.ld_r2_given = true;
    }
    else if (a == "--ld-output-path") c.ld_output_path = one(i);
    else if (a == "--grm-ld-window") {
      const std::string v = one(i);
      char* end = nullptr;
      const long w = std::strtol(v.c_str(), &end, 10);
      if (v.empty() || *end || w < 0 || w > PCOA_LD_MAX_WINDOW)
        die("--grm-ld-window (the LD pruning of --grm) takes a number of variants in [1, " + std::to_string(PCOA_LD_MAX_WINDOW) +
            "] (0: off), not '" + v + "'");
      c.grm_ld_window = (int)w;
    }
    else if (a == "--grm-ld-r2") {
      const std::string v = one(i);
      char* end = nullptr;
      c.grm_ld_r2 = std::strtod(v.c_str(), &end);
      if (v.empty() || *end || !(c.grm_ld_r2 >= 0.0 && c.grm_ld_r2 <= 1.0))
        die("--grm-ld-r2 (the threshold of --grm-ld-window) takes a value in [0, 1], not '" + v + "'");
      c.grm_ld_r2_given = true;
    }
    else if (a == "--grm-ld-output-path") c.grm_ld_output_path = one(i);
    else if (a == "--parse-only") c.parse_only = true;
    else if (a == "--dump-similarity") c.dump_similarity = one(i);
    else if (a == "--ingest-threads") c.ingest_threads = std::atoi(one(i).c_str());
    else if (a == "--plink-ref-allele") {
      c.plink_ref_allele = one(i);
      if (c.plink_ref_allele != "a1" && c.plink_ref_allele != "a2") die("--plink-ref-allele takes a1 or a2");
    }
    else die("unknown flag " + a);
  }
  if (c.gpus < 1) die("--gpus must be >= 1");
  if (c.gpu_map.empty())
    for (int g = 0; g < c.gpus; ++g) c.gpu_map.push_back(c.gpu + g);
  if ((int)c.gpu_map.size() != c.gpus) die("--gpu-map must name exactly --gpus devices");
  if (c.reduce != "auto" && c.reduce != "rccl" && c.reduce != "peer" && c.reduce != "scatter")
    die("--reduce takes auto, rccl, peer or scatter");
  if (c.layout != "auto" && c.layout != "full" && c.layout != "strips") die("--layout takes auto, full or strips");
  if (c.layout == "strips" && c.reduce == "rccl") die("--layout strips has no reduction step: it cannot take --reduce rccl");
  if (c.plink_decode != "device" && c.plink_decode != "host") die("--plink-decode takes device or host");
  if (c.stream_rows < 1) die("--stream-rows must be >= 1");
  // --grm: one GRM engine holds the 2-bit genotypes of one PLINK fileset: what needs S, carrier bitsets or several engines is
  // refused here, before any file is read or any engine exists, in a message that names --grm and the other flag
  if (!c.grm && c.has_grm_min_maf) die("--grm-min-maf needs --grm (the standardised-genotype PCA is off without it)");
  {
    const char* why = " needs --grm (it is quality control on the genotype store of the standardised-genotype PCA)";
    if (!c.grm && c.has_grm_geno) die(std::string("--grm-geno") + why);
    if (!c.grm && c.has_grm_hwe) die(std::string("--grm-hwe") + why);
    if (!c.grm && c.has_grm_mind) die(std::string("--grm-mind") + why);
    if (!c.grm && !c.grm_variant_qc_output_path.empty()) die(std::string("--grm-variant-qc-output-path") + why);
    if (!c.grm && !c.grm_sample_qc_output_path.empty()) die(std::string("--grm-sample-qc-output-path") + why);
  }
  if (!c.grm && !c.grm_weights_output_path.empty())
    die("--grm-weights-output-path needs --grm (the SNP weights are those of the axes of K; the loadings of the carrier counts go to "
        "--loadings-output-path)");
  if (!c.grm && !c.grm_project_path.empty())
    die("--grm-project-path needs --grm (it places a second PLINK fileset on the axes of K; VCFs are placed on the principal "
        "coordinates of S by --project-input-path)");
  if (!c.grm && !c.grm_output_path.empty())
    die("--grm-output-path needs --grm (it writes the relationship matrix K of the standardised genotypes; the shared counts S go to "
        "--dump-similarity)");
  if (!c.grm && c.has_grm_output_divisor) die("--grm-output-divisor needs --grm (and --grm-output-path)");
  {
    const char* why = " needs --grm (it screens the relationship matrix K of the standardised genotypes; a stored similarity matrix is "
                      "screened by --related-min-jaccard / --king-cutoff)";
    if (!c.grm && c.grm_cutoff_given) die(std::string("--grm-cutoff") + why);
    if (!c.grm && c.has_grm_cutoff_divisor) die(std::string("--grm-cutoff-divisor") + why);
    if (!c.grm && c.has_grm_related_output_path) die(std::string("--grm-related-output-path") + why);
    if (!c.grm && c.grm_cutoff_remove) die(std::string("--grm-cutoff-remove") + why);
  }
  {
    const char* why = " needs --grm (it screens the genotype store of the standardised-genotype PCA by KING-robust kinship; a stored "
                      "similarity matrix is screened by --king-cutoff)";
    if (!c.grm && c.grm_king) die(std::string("--grm-king-cutoff") + why);
    if (!c.grm && c.has_grm_king_rows) die(std::string("--grm-king-rows") + why);
    if (!c.grm && c.has_grm_king_output_path) die(std::string("--grm-king-output-path") + why);
    if (!c.grm && c.grm_king_max_pairs_given) die(std::string("--grm-king-max-pairs") + why);
    if (!c.grm && c.grm_king_remove) die(std::string("--grm-king-remove") + why);
  }
  {
    const char* why = " needs --grm (it estimates PC-Relate kinship on the genotype store and the axes of the standardised-genotype PCA)";
    if (!c.grm && c.has_grm_pcrelate_output_path) die(std::string("--grm-pcrelate-output-path") + why);
    if (!c.grm && c.has_grm_pcrelate_pcs) die(std::string("--grm-pcrelate-pcs") + why);
    if (!c.grm && c.has_grm_pcrelate_cutoff) die(std::string("--grm-pcrelate-cutoff") + why);
    if (!c.grm && c.has_grm_pcrelate_maf_threshold) die(std::string("--grm-pcrelate-maf-threshold") + why);
    if (!c.grm && c.has_grm_pcrelate_inbreeding_output_path) die(std::string("--grm-pcrelate-inbreeding-output-path") + why);
    if (!c.grm && c.grm_pcrelate_max_pairs_given) die(std::string("--grm-pcrelate-max-pairs") + why);
  }
  {
    const char* why = " needs --grm (it prunes the genotype store of the standardised-genotype PCA; the carrier counts S are pruned by --ld-window)";
    if (!c.grm && c.grm_ld_window != 0) die(std::string("--grm-ld-window") + why);
    if (!c.grm && c.grm_ld_r2_given) die(std::string("--grm-ld-r2") + why);
    if (!c.grm && !c.grm_ld_output_path.empty()) die(std::string("--grm-ld-output-path") + why);
    if (c.grm_ld_window == 0 && c.grm_ld_r2_given) die("--grm-ld-r2 needs --grm-ld-window W (the pruning is off without it)");
    if (c.grm_ld_window == 0 && !c.grm_ld_output_path.empty()) die("--grm-ld-output-path needs --grm-ld-window W (the pruning is off without it)");
  }
  {
    const char* why = " needs --grm (it subsets the genotype store of the standardised-genotype PCA; a stored similarity matrix is subset by "
                      "--outlier-iterations / --remove-related)";
    if (!c.grm && !c.grm_keep_samples.empty()) die(std::string("--grm-keep-samples") + why);
    if (!c.grm && !c.grm_remove_samples.empty()) die(std::string("--grm-remove-samples") + why);
    if (!c.grm && c.grm_outlier_iterations != 0) die(std::string("--grm-outlier-iterations") + why);
    if (!c.grm && c.grm_outlier_sigma_given) die(std::string("--grm-outlier-sigma") + why);
    if (!c.grm && c.grm_project_removed) die(std::string("--grm-project-removed") + why);
    if (!c.grm && c.grm_project_lsq)
      die("--grm-project-lsq needs --grm (it is the least-squares form of --grm-project-path / --grm-project-removed, which place samples on "
          "the axes of K)");
    if (c.grm_project_lsq && c.grm_project_path.empty() && !c.grm_project_removed)
      die("--grm-project-lsq needs --grm-project-path or --grm-project-removed (it chooses how their samples are placed)");
    if (c.grm_project_lsq && c.num_pc > 16)
      die("--grm-project-lsq takes at most 16 principal components, not " + std::to_string(c.num_pc) +
          " (pcoa_grm_project_lsq solves a system of that order per sample)");
    if (!c.grm_keep_samples.empty() && !c.grm_remove_samples.empty())
      die("--grm-keep-samples and --grm-remove-samples exclude each other (one list names the cohort)");
    if (c.grm_outlier_iterations < 0) die("--grm-outlier-iterations must be >= 0 (0 = off)");
    if (!(c.grm_outlier_sigma > 0) || !std::isfinite(c.grm_outlier_sigma))
      die("--grm-outlier-sigma must be a finite number > 0 (the threshold of --grm-outlier-iterations)");
  }
  if (!c.grm_cutoff_given) {
    const char* why = " needs --grm-cutoff X (the screen is off without it)";
    if (c.has_grm_cutoff_divisor) die(std::string("--grm-cutoff-divisor") + why);
    if (c.has_grm_related_output_path) die(std::string("--grm-related-output-path") + why);
    if (c.grm_cutoff_remove) die(std::string("--grm-cutoff-remove") + why);
  } else {
    if (!std::isfinite(c.grm_cutoff)) die("--grm-cutoff must be a finite number (the K at or above which a pair is reported)");
    if (c.has_grm_cutoff_divisor && c.grm_cutoff_divisor != "used" && c.grm_cutoff_divisor != "pairwise")
      die("--grm-cutoff-divisor takes used or pairwise, not '" + c.grm_cutoff_divisor + "'");
  }
  if (!c.grm_king) {
    const char* why = " needs --grm-king-cutoff X (the screen is off without it)";
    if (c.has_grm_king_rows) die(std::string("--grm-king-rows") + why);
    if (c.has_grm_king_output_path) die(std::string("--grm-king-output-path") + why);
    if (c.grm_king_max_pairs_given) die(std::string("--grm-king-max-pairs") + why);
    if (c.grm_king_remove) die(std::string("--grm-king-remove") + why);
  } else {
    if (!(c.grm_king_cutoff > 0 && c.grm_king_cutoff <= 0.5)) die("--grm-king-cutoff must be a finite number in (0, 0.5]");
    if (c.has_grm_king_rows && c.grm_king_rows != "all" && c.grm_king_rows != "used")
      die("--grm-king-rows takes all or used, not '" + c.grm_king_rows + "'");
    if (c.grm_king_max_pairs < 0) die("--grm-king-max-pairs must be >= 0 (the pairs --grm-king-cutoff may report)");
    if (c.grm_king_remove && c.grm_cutoff_remove)
      die("--grm-king-remove and --grm-cutoff-remove exclude each other (one relatedness screen removes samples per run)");
  }
  if (!c.has_grm_pcrelate_output_path) {
    const char* why = " needs --grm-pcrelate-output-path FILE (PC-Relate is off without it)";
    if (c.has_grm_pcrelate_pcs) die(std::string("--grm-pcrelate-pcs") + why);
    if (c.has_grm_pcrelate_cutoff) die(std::string("--grm-pcrelate-cutoff") + why);
    if (c.has_grm_pcrelate_maf_threshold) die(std::string("--grm-pcrelate-maf-threshold") + why);
    if (c.has_grm_pcrelate_inbreeding_output_path) die(std::string("--grm-pcrelate-inbreeding-output-path") + why);
    if (c.grm_pcrelate_max_pairs_given) die(std::string("--grm-pcrelate-max-pairs") + why);
  } else {
    const int most = std::min(8, c.num_pc);
    if (c.has_grm_pcrelate_pcs && !(c.grm_pcrelate_pcs >= 1 && c.grm_pcrelate_pcs <= most))
      die("--grm-pcrelate-pcs must be an integer in [1, " + std::to_string(most) + "] (min(8, --num-pc)), not " +
          std::to_string(c.grm_pcrelate_pcs));
    if (!std::isfinite(c.grm_pcrelate_cutoff))
      die("--grm-pcrelate-cutoff must be a finite number (the kinship at or above which a pair is reported)");
    if (!(c.grm_pcrelate_maf_threshold >= 0.0 && c.grm_pcrelate_maf_threshold < 0.5))
      die("--grm-pcrelate-maf-threshold must be a number in [0, 0.5)");
    if (c.grm_pcrelate_max_pairs < 0) die("--grm-pcrelate-max-pairs must be >= 0 (the pairs --grm-pcrelate-output-path may report)");
    if (!c.has_grm_pcrelate_pcs) c.grm_pcrelate_pcs = std::min(2, c.num_pc);
  }
  if (c.has_grm_output_divisor && c.grm_output_divisor != "used" && c.grm_output_divisor != "pairwise")
    die("--grm-output-divisor takes used or pairwise, not '" + c.grm_output_divisor + "'");
  if (c.has_grm_output_divisor && c.grm_output_path.empty())
    die("--grm-output-divisor needs --grm-output-path (it chooses the divisor of the matrix written there)");
  if (c.grm) {
    if (c.gpus > 1) die("--grm runs on one GRM engine: it cannot take --gpus " + std::to_string(c.gpus));
    if (c.layout == "strips") die("--grm holds no similarity matrix to tile: it cannot take --layout strips");
    if (c.gram == "implicit") die("--grm is an operator of its own over 2-bit genotypes: it cannot take --gram implicit");
    if (!c.project_input_path.empty()) die("--grm places a second PLINK fileset on the axes of K with --grm-project-path: it cannot take --project-input-path");
    if (!c.dump_similarity.empty()) die("--grm never forms a matrix: it cannot take --dump-similarity");
    if (c.similarity_measure != "shared")
      die("--grm decomposes K, not a measure over the shared counts: it cannot take --similarity-measure " + c.similarity_measure);
    if (c.missing_calls != "ignore") die("--grm mean-imputes missing calls itself: it cannot take --missing-calls " + c.missing_calls);
    if (c.outlier_iterations != 0) die("--grm holds no matrix to subset: it cannot take --outlier-iterations");
    if (c.related) die("--grm holds no shared counts to screen: it cannot take --related-min-jaccard");
    if (c.king) die("--grm holds no genotype-class matrices to screen: it cannot take --king-cutoff");
    if (c.ld_window > 0)
      die("--grm prunes its genotype store by dosage r^2 with --grm-ld-window: it cannot take --ld-window (the carrier-indicator pruner "
          "in front of an accumulation)");
    if (!c.loadings_output_path.empty()) die("--grm writes the SNP weights of K with --grm-weights-output-path: it cannot take --loadings-output-path");
    if (c.carrier_format == "lists") die("--grm stores 2-bit genotypes: it cannot take --carrier-format lists");
    const std::string ext = c.input_path.size() == 1 && c.input_path[0].size() >= 4 ? c.input_path[0].substr(c.input_path[0].size() - 4) : "";
    if (c.has_maf || (ext != ".bed" && ext != ".bim" && ext != ".fam"))
      die("--grm reads the genotypes of one PLINK fileset: --input-path must name a single .bed / .bim / .fam (dosages from VCF "
          "ingest are not built)");
    if (c.no_stream) die("--grm feeds the streamed .bed blocks to the engine: it cannot take --no-stream");
    if (c.parse_only) die("--grm runs on the device: it cannot take --parse-only");
    if (c.plink_decode == "host") die("--grm keeps the genotypes as they lie in the file: it cannot take --plink-decode host");
    c.layout = "full";
  }
  // --outlier-iterations: what cannot be served is refused here, before any file is read or any engine exists
  if (c.outlier_iterations < 0) die("--outlier-iterations must be >= 0 (0 = off)");
  if (!(c.outlier_sigma > 0) || !std::isfinite(c.outlier_sigma))
    die("--outlier-sigma must be a finite number > 0 (the threshold of --outlier-iterations)");
  if (c.outlier_iterations > 0) {
    if (c.gram == "implicit") die("--outlier-iterations subsets a stored similarity matrix: it cannot take --gram implicit");
    if (c.layout == "strips") die(kStripsRefuseOutliers);
    if (!c.project_input_path.empty()) die("--outlier-iterations decomposes the cohort it is given: it cannot take --project-input-path");
  }
  // --related-min-jaccard and its companions: likewise
  if (!c.related) {
    if (!c.related_output_path.empty()) die("--related-output-path needs --related-min-jaccard X (the screen is off without it)");
    if (c.related_max_pairs_given) die("--related-max-pairs needs --related-min-jaccard X (the screen is off without it)");
    if (c.remove_related) die("--remove-related needs --related-min-jaccard X (the screen is off without it)");
  } else {
    if (!(c.related_min_jaccard > 0 && c.related_min_jaccard <= 1)) die("--related-min-jaccard must be a finite number in (0, 1]");
    if (c.related_max_pairs < 0) die("--related-max-pairs must be >= 0 (the pairs --related-min-jaccard may report)");
    if (c.gram == "implicit") die("--related-min-jaccard screens a stored similarity matrix: it cannot take --gram implicit");
    if (c.layout == "strips") die(kStripsRefuseRelated);
    if (!c.project_input_path.empty()) die("--related-min-jaccard screens the cohort it decomposes: it cannot take --project-input-path");
  }
  // --king-cutoff and its companions: likewise, naming both flags
  if (!c.king) {
    if (!c.king_output_path.empty()) die("--king-output-path needs --king-cutoff X (the screen is off without it)");
    if (c.king_max_pairs_given) die("--king-max-pairs needs --king-cutoff X (the screen is off without it)");
    if (c.king_remove) die("--king-remove needs --king-cutoff X (the screen is off without it)");
  } else {
    if (!(c.king_cutoff > 0 && c.king_cutoff <= 0.5)) die("--king-cutoff must be a finite number in (0, 0.5]");
    if (c.king_max_pairs < 0) die("--king-max-pairs must be >= 0 (the pairs --king-cutoff may report)");
    if (c.gram == "implicit") die("--king-cutoff screens stored Gram matrices: it cannot take --gram implicit");
    if (c.layout == "strips") die(kStripsRefuseKing);
    if (c.gpus > 1) die("--king-cutoff runs on one engine and its five planes: it cannot take --gpus " + std::to_string(c.gpus));
    if (c.ld_window > 0) die("--king-cutoff: the planes would need the pruned rows: it cannot take --ld-window");
    if (c.related) die("--king-cutoff: one relatedness screen per run: it cannot take --related-min-jaccard");
    if (!c.project_input_path.empty()) die("--king-cutoff screens the cohort it decomposes: it cannot take --project-input-path");
    const std::string ext = c.input_path.size() == 1 && c.input_path[0].size() >= 4 ? c.input_path[0].substr(c.input_path[0].size() - 4) : "";
    if (c.has_maf || (ext != ".bed" && ext != ".bim" && ext != ".fam"))
      die("--king-cutoff reads the genotype classes of one PLINK fileset: --input-path must name a single .bed / .bim / .fam "
          "(VCF ingest yields carriers only)");
    if (c.no_stream) die("--king-cutoff feeds the streamed .bed blocks to the five planes: it cannot take --no-stream");
    if (c.parse_only) die("--king-cutoff runs on the device: it cannot take --parse-only");
    if (c.plink_decode == "host") die("--king-cutoff decodes the five planes on the device: it cannot take --plink-decode host");
  }
  // --similarity-measure jaccard | cosine: likewise
  if (c.similarity_measure != "shared") {
    const std::string& m = c.similarity_measure;
    if (c.gram == "implicit") die("--similarity-measure " + m + " is evaluated from a stored similarity matrix: it cannot take --gram implicit");
    if (c.layout == "strips") die(strips_refuse_measure(m));
    if (!c.project_input_path.empty())
      die("--similarity-measure " + m + ": projection under a measure is not built: it cannot take --project-input-path");
  }
  // --loadings-output-path: the identity B = (X J)^T (X J) behind the loadings holds for the shared counts of the whole cohort
  // on one engine: likewise
  // --missing-calls pairwise: likewise, naming both flags
  if (c.missing_calls != "pairwise") {
    if (!c.call_rate_output_path.empty()) die("--call-rate-output-path needs --missing-calls pairwise");
  } else {
    if (c.gram == "implicit") die("--missing-calls pairwise is evaluated from two stored similarity matrices: it cannot take --gram implicit");
    if (c.layout == "strips") die(kStripsRefuseMissing);
    if (c.gpus > 1) die("--missing-calls pairwise runs on one engine and its companion: it cannot take --gpus " + std::to_string(c.gpus));
    if (!c.project_input_path.empty())
      die("--missing-calls pairwise: projection under the pairwise-complete similarity is not built: it cannot take --project-input-path");
    if (c.similarity_measure != "shared")
      die("--missing-calls pairwise: its combination with a measure is not built: it cannot take --similarity-measure " + c.similarity_measure);
    if (c.ld_window > 0) die("--missing-calls pairwise: LD pruning in front of a paired accumulation is not built: it cannot take --ld-window");
    if (!c.loadings_output_path.empty())
      die("--missing-calls pairwise: the decomposed matrix is no longer (X J)^T (X J): it cannot take --loadings-output-path");
    const std::string ext = c.input_path.size() == 1 && c.input_path[0].size() >= 4 ? c.input_path[0].substr(c.input_path[0].size() - 4) : "";
    if (c.has_maf || (ext != ".bed" && ext != ".bim" && ext != ".fam"))
      die("--missing-calls pairwise reads the missing calls of one PLINK fileset: --input-path must name a single .bed / .bim / .fam "
          "(missing calls from VCF ingest are not built)");
    if (c.no_stream) die("--missing-calls pairwise feeds the streamed .bed blocks to two engines: it cannot take --no-stream");
    if (c.parse_only) die("--missing-calls pairwise runs on the device: it cannot take --parse-only");
    if (c.plink_decode == "host") die("--missing-calls pairwise decodes both bitsets on the device: it cannot take --plink-decode host");
  }
  if (!c.loadings_output_path.empty()) {
    if (c.gpus > 1) die("--loadings-output-path streams the variants past one engine: it cannot take --gpus " + std::to_string(c.gpus));
    if (c.layout == "strips") die("--loadings-output-path runs on one whole engine: it cannot take --layout strips");
    if (!c.project_input_path.empty())
      die("--loadings-output-path writes the loadings of the cohort it decomposes: it cannot take --project-input-path");
    if (c.outlier_iterations > 0)
      die("--loadings-output-path needs the eigenpairs of the cohort the variants were counted over: it cannot take --outlier-iterations " +
          std::to_string(c.outlier_iterations));
    if (c.remove_related)
      die("--loadings-output-path needs the eigenpairs of the cohort the variants were counted over: it cannot take --remove-related");
    if (c.similarity_measure != "shared")
      die("--loadings-output-path: under --similarity-measure " + c.similarity_measure +
          " the decomposed matrix is no longer (X J)^T (X J); it takes --similarity-measure shared only");
    if (c.parse_only) die("--loadings-output-path needs the decomposition: it cannot take --parse-only");
  }
  // --ld-window: the windows run over the variants in feed order on one engine: likewise
  if (c.ld_window == 0) {
    if (!c.ld_output_path.empty()) die("--ld-output-path needs --ld-window W (the pruning is off without it)");
    if (c.ld_r2_given) die("--ld-r2 needs --ld-window W (the pruning is off without it)");
  } else {
    if (c.gpus > 1) die("--ld-window: variant shards would cut the windows: it cannot take --gpus " + std::to_string(c.gpus));
    if (c.layout == "strips") die("--ld-window runs in front of one engine's accumulation: it cannot take --layout strips");
    if (c.input_path.size() > 1)
      die("--ld-window takes one input set: joined and merged sets reach the engine in hash-partition order, not in feed order");
    if (!c.project_input_path.empty()) die("--ld-window prunes the cohort it decomposes: it cannot take --project-input-path");
    if (c.carrier_format == "lists") die("--ld-window prunes carrier bitsets: it cannot take --carrier-format lists");
    if (c.parse_only) die("--ld-window runs on the device: it cannot take --parse-only");
    if (!c.loadings_output_path.empty() && c.gram == "implicit")
      die("--loadings-output-path with --ld-window writes a line for every variant read, pruned or not, and the store of --gram implicit "
          "holds the kept ones only: use a stored S over one streamed PLINK fileset");
    c.carrier_format = "bits";
    c.layout = "full";
  }
  if (c.gram == "implicit") {
    // one operator engine holds the carrier bitsets of every variant: what needs S, or several engines, is refused here,
    // before any file is read or any engine exists
    if (c.gpus > 1) die("--gram implicit runs on one operator engine: it cannot take --gpus " + std::to_string(c.gpus));
    if (c.layout == "strips") die("--gram implicit holds no similarity matrix to tile: it cannot take --layout strips");
    if (!c.project_input_path.empty()) die("--gram implicit holds no similarity matrix to project against: it cannot take --project-input-path");
    if (c.carrier_format == "lists") die("--gram implicit stores carrier bitsets: it cannot take --carrier-format lists");
    if (!c.dump_similarity.empty()) die("--gram implicit never forms the similarity matrix: it cannot take --dump-similarity");
    c.carrier_format = "bits";
    c.layout = "full";
  }
  return c;
}

// ---- Double.toString (what Scala's string interpolation prints, :239) --------------------------
template <typename T>  // T = double: Double.toString; T = float: Float.toString (same layout rules)
std::string java_number(T d) {
  if (std::isnan(d)) return "NaN";
  if (std::isinf(d)) return d > 0 ? "Infinity" : "-Infinity";
  if (d == 0) return std::signbit(d) ? "-0.0" : "0.0";
  char buf[64];
  auto r = std::to_chars(buf, buf + sizeof(buf), std::fabs(d), std::chars_format::scientific);  // shortest round trip
  std::string s(buf, r.ptr);                      // d.ddddde[+-]XX
  const size_t epos = s.find('e');
  std::string mant = s.substr(0, epos);
  int e10 = std::atoi(s.c_str() + epos + 1);
  std::string digits;
  for (char ch : mant)
    if (ch != '.') digits.push_back(ch);
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  const std::string sign = d < 0 ? "-" : "";
  const double ad = std::fabs(d);
  if (ad >= 1e-3 && ad < 1e7) {
    std::string whole, frac;
    if (e10 >= 0) {
      whole = digits.substr(0, std::min<size_t>(digits.size(), (size_t)e10 + 1));
      while ((int)whole.size() < e10 + 1) whole.push_back('0');
      frac = digits.size() > (size_t)e10 + 1 ? digits.substr((size_t)e10 + 1) : "0";
    } else {
      whole = "0";
      frac = std::string((size_t)(-e10 - 1), '0') + digits;
    }
    return sign + whole + "." + frac;
  }
  return sign + digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(e10);
}
std::string java_double(double d) { return java_number<double>(d); }

// ---- Guava Hashing.murmur3_128().hashBytes(..).toString() -------------------------------------
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix64(uint64_t k) {
  k ^= k >> 33; k *= 0xFF51AFD7ED558CCDULL; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ULL; k ^= k >> 33;
  return k;
}
std::string murmur3_128_hex(const std::string& data) {
  const uint64_t c1 = 0x87C37B91114253D5ULL, c2 = 0x4CF5AD432745937FULL;
  uint64_t h1 = 0, h2 = 0;
  const size_t n = data.size(), nblocks = n / 16;
  auto rd = [&](size_t off, size_t len) { uint64_t v = 0; std::memcpy(&v, data.data() + off, len); return v; };
  for (size_t i = 0; i < nblocks; ++i) {
    uint64_t k1 = rd(16 * i, 8), k2 = rd(16 * i + 8, 8);
    k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52DCE729;
    k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495AB5;
  }
  const size_t t = n - 16 * nblocks;
  if (t > 8) { uint64_t k2 = rd(16 * nblocks + 8, t - 8); k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2; }
  if (t > 0) { uint64_t k1 = rd(16 * nblocks, std::min<size_t>(t, 8)); k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= n; h2 ^= n; h1 += h2; h2 += h1; h1 = fmix64(h1); h2 = fmix64(h2); h1 += h2; h2 += h1;
  char out[33];
  unsigned char b[16];
  std::memcpy(b, &h1, 8); std::memcpy(b + 8, &h2, 8);  // little-endian host
  for (int i = 0; i < 16; ++i) std::snprintf(out + 2 * i, 3, "%02x", b[i]);
  return std::string(out, 32);
}

// ---- variants -------------------------------------------------------------------------------
// case class CallData(hasVariation, callsetId) (:288): everything downstream of extractCallInfo (:56-60) only ever
// keeps the calls with hasVariation (getCallsRdd :163-167; join / merge concatenate the call lists first, which
// commutes with the filter because callset indices are global), so a variant stores its CARRIERS: the callset
// indices with variation, in call order.
struct VarMeta { std::string contig; long pos = 0; std::string id; };   // a line's first columns in the --loadings-output-path file
bool g_want_meta = false;          // --loadings-output-path given: contig, position and id are recorded during ingest (only then)
// --ld-window: every row on its way to the engine goes through the pruner (PCOA_LD_ACCUMULATE) instead of pcoa_accumulate_bits /
// pcoa_accumulate_plink_bed, with a pcoa_ld_break wherever the contig of the next variant differs from the last one's
struct LdFeed {
  bool on = false;
  const std::vector<VarMeta>* meta = nullptr;   // of every row fed so far and of the rows of the call being made, in feed order
  std::vector<uint8_t> keep;                    // one flag per fed row
  int64_t fed = 0;
  std::string last_contig;
  // rows [a, b) of a call share a contig: run(a, b, keep_out)
  void rows_in(pcoa_ctx* ctx, int64_t rows, const std::function<void(int64_t, int64_t, uint8_t*)>& run) {
    keep.resize((size_t)(fed + rows));
    const bool known = meta && (int64_t)meta->size() >= fed + rows;
    for (int64_t a = 0; a < rows;) {
      int64_t b = rows;
      if (known) {
        const std::string& contig = (*meta)[(size_t)(fed + a)].contig;
        for (b = a + 1; b < rows && (*meta)[(size_t)(fed + b)].contig == contig; ++b) {}
        if (fed + a > 0 && contig != last_contig && pcoa_ld_break(ctx) != PCOA_OK) die(std::string("pcoa_ld_break: ") + pcoa_last_error(ctx));
        last_contig = contig;
      }
      run(a, b, keep.data() + fed + a);
      a = b;
    }
    fed += rows;
  }
  void bits(pcoa_ctx* ctx, const uint32_t* rows_ptr, int64_t rows, int64_t words) {
    rows_in(ctx, rows, [&](int64_t a, int64_t b, uint8_t* out) {
      if (pcoa_ld_bits(ctx, rows_ptr + a * words, b - a, words, 0, out, nullptr) != PCOA_OK) die(std::string("pcoa_ld_bits: ") + pcoa_last_error(ctx));
    });
  }
  void bed(pcoa_ctx* ctx, const unsigned char* rows_ptr, int64_t rows, int64_t bpv, int ref_a1) {
    rows_in(ctx, rows, [&](int64_t a, int64_t b, uint8_t* out) {
      if (pcoa_ld_plink_bed(ctx, rows_ptr + a * bpv, b - a, bpv, ref_a1, 0, out, nullptr) != PCOA_OK)
        die(std::string("pcoa_ld_plink_bed: ") + pcoa_last_error(ctx));
    });
  }
};
LdFeed g_ld;

// --missing-calls pairwise: the companion engine every streamed .bed block's missing-call bitsets go to
struct CallsFeed {
  bool on = false;
  pcoa_ctx* companion = nullptr;
};
CallsFeed g_calls;
// --king-cutoff: the five plane engines (PCOA_KING_*) that take the genotype-class bitsets of the same streamed .bed blocks;
// created beside engine 0, destroyed right after the screen
struct KingFeed {
  bool on = false;
  pcoa_ctx* planes[PCOA_KING_PLANES] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};
KingFeed g_king;
struct Variant {
  std::string key;                 // getVariantKey
  VarMeta meta;                    // (g_want_meta)
  bool has_af = false; float af = 0.f;
  std::vector<int32_t> carriers;   // extractCallInfo (:56-60) filtered by hasVariation
};
struct Dataset {
  std::vector<std::string> ids, names;
  std::vector<Variant> variants;
};

// contig normalisation of the reference (VariantsRDD.scala:103-110): [a-z]*[0-9]+ -> the number
bool normalize_contig(const std::string& name, std::string& out) {
  size_t i = 0;
  while (i < name.size() && std::isalpha((unsigned char)name[i])) ++i;
  if (i == name.size()) return false;
  for (size_t j = i; j < name.size(); ++j)
    if (!std::isdigit((unsigned char)name[j])) return false;
  out = name.substr(i);
  return true;
}

struct Region { std::string contig; long start, end; };
std::vector<Region> parse_references(const std::string& spec) {
  std::vector<Region> out;
  std::stringstream ss(spec);
  std::string tup;
  while (std::getline(ss, tup, ',')) {
    if (tup.empty()) continue;
    const size_t a = tup.find(':'), b = tup.rfind(':');
    if (a == std::string::npos || a == b) die("bad --references tuple " + tup);
    Region r;
    std::string ctg = tup.substr(0, a);
    if (!normalize_contig(ctg, r.contig)) r.contig = ctg;
    r.start = std::atol(tup.substr(a + 1, b - a - 1).c_str());
    r.end = std::atol(tup.substr(b + 1).c_str());
    out.push_back(r);
  }
  return out;
}

// ---- VCF ingest ------------------------------------------------------------------------------------------------
// The file (or the output of `gzip -dc`) is read in 16 MiB blocks cut at line ends; the data lines of a block are
// parsed by a pool of threads (contiguous line ranges, results concatenated in file order), in place with
// string_views: no per-field allocation.  One sample column costs a scan up to the next tab.
struct BlockReader {  // plain file, or the output of `gzip -dc -- <path>` started with posix_spawn (no shell: the
                      // path is one argv entry, whatever characters it holds)
  FILE* f = nullptr;
  pid_t child = -1;
  std::string carry;
  explicit BlockReader(const std::string& path) {
    if (path.size() > 3 && path.substr(path.size() - 3) == ".gz") {
      int fds[2];
      if (pipe(fds) != 0) die("pipe() failed for " + path);
      posix_spawn_file_actions_t fa;
      posix_spawn_file_actions_init(&fa);
      posix_spawn_file_actions_adddup2(&fa, fds[1], STDOUT_FILENO);
      posix_spawn_file_actions_addclose(&fa, fds[0]);
      posix_spawn_file_actions_addclose(&fa, fds[1]);
      std::string a0 = "gzip", a1 = "-dc", a2 = "--", a3 = path;
      char* argv[] = {a0.data(), a1.data(), a2.data(), a3.data(), nullptr};
      const int rc = posix_spawnp(&child, "gzip", &fa, nullptr, argv, environ);
      posix_spawn_file_actions_destroy(&fa);
      close(fds[1]);
      if (rc != 0) { close(fds[0]); die("cannot start gzip for " + path); }
      f = fdopen(fds[0], "r");
    } else {
      f = std::fopen(path.c_str(), "r");
    }
    if (!f) die("cannot open " + path);
  }
  ~BlockReader() {
    if (f) std::fclose(f);
    if (child > 0) { int st = 0; (void)waitpid(child, &st, 0); }
  }
  // next block of whole lines (the last one may lack its newline at end of file); false at end of input
  bool next(std::string& block, size_t target = (size_t)16 << 20) {
    block.swap(carry);
    carry.clear();
    for (;;) {
      const size_t old = block.size();
      block.resize(old + target);
      const size_t got = std::fread(&block[old], 1, target, f);
      block.resize(old + got);
      if (got == 0) return !block.empty();
      const size_t nl = block.rfind('\n');
      if (nl != std::string::npos) {
        carry.assign(block, nl + 1, std::string::npos);
        block.resize(nl + 1);
        return true;
      }
    }
  }
};

inline std::string_view next_field(const char*& p, const char* end, char sep) {
  const char* b = p;
  const char* e = static_cast<const char*>(std::memchr(p, sep, (size_t)(end - p)));
  if (!e) { p = end; return std::string_view(b, (size_t)(end - b)); }
  p = e + 1;
  return std::string_view(b, (size_t)(e - b));
}

struct ParsedLine { bool keep = false; Variant v; std::string debug; };
double g_ingest_read_s = 0, g_ingest_split_s = 0, g_ingest_parse_s = 0;  // --parse-only breakdown
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void parse_record(const char* b, const char* e, const std::vector<Region>& regions, int32_t index_base, size_t n_samples,
                  bool debug, ParsedLine& out) {
  const char* p = b;
  std::string_view f[9];
  for (int i = 0; i < 9; ++i) {
    if (p >= e) return;  // fewer than 10 columns
    f[i] = next_field(p, e, '\t');
  }
  if (p >= e) return;
  std::string contig;
  if (!normalize_contig(std::string(f[0]), contig)) return;  // X, Y, MT ... dropped as in the reference
  const long start = std::atol(std::string(f[1]).c_str()) - 1;
  if (!regions.empty()) {
    bool in_region = false;
    for (const auto& r : regions) in_region = in_region || (r.contig == contig && r.start <= start && start < r.end);
    if (!in_region) return;
  }
  int gti = -1, k = 0;
  for (const char *q = f[8].data(), *qe = q + f[8].size(); q < qe; ++k)
    if (next_field(q, qe, ':') == "GT") gti = k;
  if (gti < 0) return;
  Variant& v = out.v;
  std::string alt;
  for (const char *q = f[4].data(), *qe = q + f[4].size(); q < qe;) {
    const std::string_view a = next_field(q, qe, ',');
    if (a != ".") alt.append(a);
  }
  const long end = start + (long)f[3].size();
  if (debug) {
    char line[512];
    std::snprintf(line, sizeof(line), "%s: (%ld, %ld) ref=%.*s alt=%s\n", contig.c_str(), start, end, (int)f[3].size(),
                  f[3].data(), alt.c_str());
    out.debug = line;
  }
  std::string buf = contig;
  int64_t s64 = start, e64 = end;
  buf.append(reinterpret_cast<const char*>(&s64), 8);
  buf.append(reinterpret_cast<const char*>(&e64), 8);
  buf.append(f[3]);
  buf += alt;
  v.key = murmur3_128_hex(buf);
  if (g_want_meta) v.meta = VarMeta{contig, start + 1, std::string(f[2])};
  for (const char *q = f[7].data(), *qe = q + f[7].size(); q < qe;) {
    const std::string_view item = next_field(q, qe, ';');
    if (item.size() >= 3 && item.compare(0, 3, "AF=") == 0) {
      v.af = std::strtof(std::string(item.substr(3)).c_str(), nullptr);
      v.has_af = true;
    }
  }
  // sample columns: one pass over the bytes.  A call has variation iff a digit 1-9 occurs inside its GT sub-field
  // (sub-field number gti of the ':'-separated column) -- genotype.foldLeft(false)(_ || _ > 0) (:58): "." and "0"
  // alleles do not count, phasing marks are irrelevant.
  v.carriers.reserve(64);
  for (size_t i = 0; i < n_samples && p < e; ++i) {
    bool var = false;
    int col = 0;
    for (; p < e; ++p) {
      const char c = *p;
      if (c == '\t') break;
      if (c == ':') { ++col; continue; }
      var |= (col == gti) & (c >= '1') & (c <= '9');
    }
    if (p < e) ++p;  // past the tab
    if (var) v.carriers.push_back(index_base + (int32_t)i);
  }
  out.keep = true;
}

// Set id of a VCF = its file name up to the first '.', '-' replaced (the id is split at '-' for the dataset column,
// :235).  Two files with the same stem (a/cohort.chr17.vcf + b/cohort.chr17.vcf, ALL.chr17.phase1 + ALL.chr17.phase3)
// would collide: the later one gets "<stem>_<ordinal>" -- the same rule as the Python mirror (load_dataset).
std::string set_id_of(const std::string& path, size_t ordinal, std::set<std::string>& used) {
  std::string stem = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
  stem = stem.substr(0, stem.find('.'));
  std::replace(stem.begin(), stem.end(), '-', '_');
  if (used.count(stem)) stem += "_" + std::to_string(ordinal);
  used.insert(stem);
  return stem;
}

// sink: called with every block's parsed records instead of keeping them (a single VCF is fed block by block, r05);
// header_only: stop behind the #CHROM line (ids / names only).
Dataset load_vcf(const std::string& path, const std::string& stem, const std::vector<Region>& regions, int32_t index_base,
                 bool debug, int n_threads, const std::function<void(std::vector<ParsedLine>&)>* sink = nullptr,
                 bool header_only = false) {
  Dataset d;
  BlockReader in(path);
  std::string block;
  bool header = false;
  if (n_threads <= 0) n_threads = (int)std::max(1u, std::thread::hardware_concurrency());
  for (;;) {
    double t0 = now_s();
    if (!in.next(block)) break;
    g_ingest_read_s += now_s() - t0;
    t0 = now_s();
    // line starts of this block; header lines are handled here, data lines go to the pool
    std::vector<std::pair<const char*, const char*>> lines;
    const char* p = block.data();
    const char* bend = p + block.size();
    while (p < bend) {
      const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(bend - p)));
      const char* le = nl ? nl : bend;
      const char* lb = p;
      p = nl ? nl + 1 : bend;
      if (le > lb && le[-1] == '\r') --le;
      if (le == lb) continue;
      if (lb[0] == '#') {
        if (le - lb >= 6 && std::memcmp(lb, "#CHROM", 6) == 0) {
          const char* q = lb;
          for (int i = 0; q < le; ++i) {
            const std::string_view col = next_field(q, le, '\t');
            if (i >= 9) {
              d.names.emplace_back(col);
              d.ids.push_back(stem + "-" + std::to_string(i - 9));
            }
          }
          header = true;
          if (header_only) return d;
        }
        continue;
      }
      if (!header) die("VCF header line (#CHROM) missing in " + path);
      lines.emplace_back(lb, le);
    }
    g_ingest_split_s += now_s() - t0;
    t0 = now_s();
    std::vector<ParsedLine> parsed(lines.size());
    const size_t nt = std::min<size_t>((size_t)n_threads, std::max<size_t>(1, lines.size() / 64));
    auto work = [&](size_t t) {
      const size_t lo = lines.size() * t / nt, hi = lines.size() * (t + 1) / nt;
      for (size_t i = lo; i < hi; ++i)
        parse_record(lines[i].first, lines[i].second, regions, index_base, d.ids.size(), debug, parsed[i]);
    };
    if (nt <= 1) {
      work(0);
    } else {
      std::vector<std::thread> pool;
      for (size_t t = 0; t < nt; ++t) pool.emplace_back(work, t);
      for (auto& th : pool) th.join();
    }
    g_ingest_parse_s += now_s() - t0;
    if (sink) {
      (*sink)(parsed);
      continue;
    }
    for (auto& pl : parsed) {
      if (!pl.keep) continue;
      if (debug) std::fputs(pl.debug.c_str(), stdout);
      d.variants.push_back(std::move(pl.v));
    }
  }
  if (!header) die("no #CHROM header in " + path);
  return d;
}

void check(pcoa_ctx* ctx, int rc, const char* what) {
  if (rc != PCOA_OK) die(std::string(what) + ": " + pcoa_last_error(ctx));
}

}  // namespace

bool is_plink_path(const std::string& p) {
  if (p.size() < 4) return false;
  const std::string ext = p.substr(p.size() - 4);
  return ext == ".bed" || ext == ".bim" || ext == ".fam";
}

// PLINK 1 binary fileset (<prefix>.bed / .bim / .fam), the twin of the Python mirror's ingest.load_plink: variant-major
// .bed, two bits per genotype, four samples to a byte (sample s in bits 2 (s % 4) of byte s / 4): 00 homozygous A1,
// 01 missing, 10 heterozygous, 11 homozygous A2.  A2 is the reference allele (plink --keep-allele-order / plink2
// --make-bed), so hasVariation (:56-60) = code 00 or 10; a missing call has none.  Callset index = row of the .fam,
// name = its IID.  Contig rule and --references filter as for a VCF (0-based start = bp - 1); a .bim names the sex and
// mitochondrial chromosomes by NUMBER (23 X, 24 Y, 25 XY, 26 MT, 0 unplaced), which the VCF rule would keep as ordinary
// contigs although the reference drops X / Y / MT (VariantsRDD.scala:103-110): they are mapped back to their names first,
// so the same cohort gives the same S through either format.  ref_a1: A1 is the reference allele (a fileset written
// without --keep-allele-order): the codes 00 and 11 trade places.
std::string plink_chrom_name(const std::string& chrom) {
  if (chrom == "23") return "X";
  if (chrom == "24") return "Y";
  if (chrom == "25") return "XY";
  if (chrom == "26") return "MT";
  if (chrom == "0") return "unplaced";
  return chrom;
}

struct PlinkMeta {
  std::string prefix;
  std::vector<std::string> ids, names;
  std::vector<char> keep;  // per .bim line: inside --references and on a contig the reference keeps
  std::vector<VarMeta> meta;   // of the kept lines, in file order (g_want_meta)
  size_t n = 0, bpv = 0;   // samples; bytes per variant row of the .bed
};

PlinkMeta read_plink_meta(const std::string& path, const std::string& stem, const std::vector<Region>& regions) {
  PlinkMeta m;
  m.prefix = path.substr(0, path.size() - 4);
  const std::string& prefix = m.prefix;
  {
    std::ifstream fam(prefix + ".fam");
    if (!fam) die("cannot open " + prefix + ".fam");
    std::string line;
    while (std::getline(fam, line)) {
      std::istringstream is(line);
      std::string fid, iid;
      if (!(is >> fid >> iid)) continue;
      m.names.push_back(iid);
      m.ids.push_back(stem + "-" + std::to_string(m.ids.size()));
    }
  }
  m.n = m.ids.size();
  if (m.n == 0) die("no samples in " + prefix + ".fam");
  {
    std::ifstream bim(prefix + ".bim");
    if (!bim) die("cannot open " + prefix + ".bim");
    std::string line;
    while (std::getline(bim, line)) {
      std::istringstream is(line);
      std::string chrom, id, cm;
      long bp = 0;
      if (!(is >> chrom >> id >> cm >> bp)) continue;
      std::string contig;
      bool ok = normalize_contig(plink_chrom_name(chrom), contig);
      if (ok && !regions.empty()) {
        ok = false;
        for (const auto& r : regions)
          if (r.contig == contig && r.start <= bp - 1 && bp - 1 < r.end) { ok = true; break; }
      }
      m.keep.push_back(ok ? 1 : 0);
      if (ok && g_want_meta) m.meta.push_back(VarMeta{contig, bp, id});
    }
  }
  m.bpv = (m.n + 3) / 4;
  // the .bed must be exactly 3 + variants * bpv bytes
  std::ifstream bed(prefix + ".bed", std::ios::binary | std::ios::ate);
  if (!bed) die("cannot open " + prefix + ".bed");
  const std::streamoff size = bed.tellg();
  bed.seekg(0);
  unsigned char magic[3] = {0, 0, 0};
  bed.read(reinterpret_cast<char*>(magic), 3);
  if (!bed || magic[0] != 0x6c || magic[1] != 0x1b) die(prefix + ".bed: not a PLINK 1 binary file");
  if (magic[2] != 1) die(prefix + ".bed is sample-major; only the variant-major layout is read");
  const std::streamoff want = 3 + (std::streamoff)(m.keep.size() * m.bpv);
  if (size < want) die(prefix + ".bed is shorter than its .bim / .fam say");
  if (size > want) die(prefix + ".bed is longer than its .bim / .fam say");
  return m;
}

// the in-memory form (r03; --no-stream, --parse-only): carrier lists of every kept variant
Dataset load_plink(const std::string& path, const std::string& stem, const std::vector<Region>& regions, int32_t index_base,
                   bool ref_a1) {
  PlinkMeta m = read_plink_meta(path, stem, regions);
  Dataset d;
  d.ids = m.ids;
  d.names = m.names;
  const size_t n = m.n, bpv = m.bpv;
  std::ifstream bed(m.prefix + ".bed", std::ios::binary);
  bed.seekg(3);
  std::vector<unsigned char> row(bpv);
  for (size_t v = 0; v < m.keep.size(); ++v) {
    bed.read(reinterpret_cast<char*>(row.data()), (std::streamsize)bpv);
    if ((size_t)bed.gcount() != bpv) die(m.prefix + ".bed is shorter than its .bim / .fam say");
    if (!m.keep[v]) continue;
    Variant var;
    if (g_want_meta) var.meta = m.meta[d.variants.size()];
    for (size_t s = 0; s < n; ++s) {
      const unsigned code = (row[s >> 2] >> (2 * (s & 3))) & 3u;
      if (code == 2u || code == (ref_a1 ? 3u : 0u)) var.carriers.push_back(index_base + (int32_t)s);
    }
    d.variants.push_back(std::move(var));
  }
  return d;
}

// ---- r04: one engine per GPU ---------------------------------------------------------------------------------------------
// Contiguous, balanced ranges: the first (total mod k) shards get one unit more (dist.shard_range of the Python host; the
// reference's partitions, VariantsPca.scala:184).
void shard_range(int g, int k, int64_t total, int64_t* b, int64_t* e) {
  const int64_t base = total / k, extra = total % k;
  *b = g * base + std::min<int64_t>(g, extra);
  *e = *b + base + (g < extra ? 1 : 0);
}

// 2-bit PLINK codes of one row -> carrier bitset words (host decode, --plink-decode host): 8 bytes = 32 samples = one word
void bed_row_to_bits(const unsigned char* row, size_t bpv, size_t n, bool ref_a1, uint32_t* out, size_t words) {
  const uint64_t E = 0x5555555555555555ull;
  for (size_t w = 0; w < words; ++w) {
    uint64_t x = 0;
    const size_t at = 8 * w, have = at < bpv ? std::min<size_t>(8, bpv - at) : 0;
    std::memcpy(&x, row + at, have);  // little-endian host
    const uint64_t lo = x & E, hi = (x >> 1) & E;
    uint64_t m = (hi & ~lo) | (ref_a1 ? (hi & lo) : (~hi & ~lo & E));
    m = (m | (m >> 1)) & 0x3333333333333333ull;
    m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
    m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
    m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
    m = (m | (m >> 16)) & 0x00000000ffffffffull;
    uint32_t keep = 0xffffffffu;
    if (32 * w >= n) keep = 0;
    else if (32 * w + 32 > n) keep = (1u << (n - 32 * w)) - 1u;
    out[w] = (uint32_t)m & keep;
  }
}

// A few reader threads that live as long as a shard is streamed (r05: eight threads created per 41-MB block cost a quarter of
// the block's feed time): run(job) hands job(t) to every thread t and returns when all are done.
class ReaderPool {
 public:
  explicit ReaderPool(unsigned n) {
    for (unsigned t = 0; t < n; ++t)
      th_.emplace_back([this, t] {
        int seen = 0;
        for (;;) {
          std::unique_lock<std::mutex> lk(mu_);
          cv_job_.wait(lk, [&] { return stop_ || gen_ != seen; });
          if (stop_) return;
          seen = gen_;
          const std::function<void(unsigned)> j = job_;
          lk.unlock();
          j(t);
          lk.lock();
          if (--pending_ == 0) cv_done_.notify_all();
        }
      });
  }
  ~ReaderPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_job_.notify_all();
    for (auto& t : th_) t.join();
  }
  unsigned size() const { return (unsigned)th_.size(); }
  void run(const std::function<void(unsigned)>& job) {
    std::unique_lock<std::mutex> lk(mu_);
    job_ = job;
    pending_ = (int)th_.size();
    ++gen_;
    cv_job_.notify_all();
    cv_done_.wait(lk, [&] { return pending_ == 0; });
  }

 private:
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_job_, cv_done_;
  std::function<void(unsigned)> job_;
  int gen_ = 0, pending_ = 0;
  bool stop_ = false;
};

struct StreamStats {
  std::mutex mu;
  int64_t variants = 0;
  double read_s = 0, feed_s = 0;
};

// Shard g of a PLINK fileset, streamed: blocks of --stream-rows variants are read (pread, own descriptor) one block ahead of
// the engine, rows outside --references squeezed out, and handed over as they lie in the file (device decode) or as bitsets
// decoded here.  Never more than four blocks in memory per engine (VariantsRDD.compute is an iterator, rdd/VariantsRDD.scala:
// 205-235; the reference never holds a data set either).
// RDD[Seq[Int]] rows -> engine (r06; VERDICT r05 Weak 7).  A carrier list costs 4 bytes per carrier, a carrier bitset N / 8 bytes
// per variant whatever the list's length: at configs[1]'s 337 carriers per variant that is 1,356 against 316 bytes, and the
// link bounds the lists at ~40 M variants/s.  Blocks whose mean list is longer than N / 32 entries are packed into bitsets --
// by `threads` host threads, chunk k + 1 while chunk k crosses -- in two page-locked buffers and handed to
// pcoa_accumulate_bits; sparse blocks, and chunks in which a list names a callset twice (the reference counts the repeat with
// multiplicity, VariantsPca.scala:187: a bitset cannot), go over as lists (pcoa_accumulate_calls_ex).
// ---- streamed joins / merges (r06; VERDICT r05 Missing 6) ----------------------------------------------------------------------
// joinDatasets / mergeDatasets are shuffles on getVariantKey (VariantsPca.scala:115-148): records with the same key meet in
// one reduce partition, and no partition ever holds a whole variant set.  The in-memory path held every set as
// std::vector<Variant> before the first row reached the engine.  Here every set is streamed ONCE (16-MiB blocks through the
// parser threads) and each kept record -- key, AF-filter verdict already applied, carriers -- is appended to the spill file of
// partition hash(key) mod P; then one partition at a time is read back, joined / merged exactly as the in-memory path does,
// and fed.  The order of the joined rows differs from the in-memory path; S is a sum over rows and does not care.
struct JoinSpill {
  std::string dir, tag;
  int sets = 0, parts = 0;
  std::vector<std::string> pending;   // per (set, partition): bytes not yet written
  std::vector<int64_t> counts;
  int64_t bytes = 0;
  std::string path(int set, int part) const { return dir + "/" + tag + "_" + std::to_string(set) + "_" + std::to_string(part) + ".bin"; }
  void open(const Conf& conf, int n_sets) {
    dir = !conf.spill_dir.empty() ? conf.spill_dir : (std::getenv("TMPDIR") && *std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp");
    tag = "pcoa_join_" + std::to_string((long long)::getpid());
    sets = n_sets;
    parts = conf.join_partitions;
    pending.assign((size_t)sets * parts, std::string());
    counts.assign((size_t)sets * parts, 0);
    for (int s = 0; s < sets; ++s)
      for (int q = 0; q < parts; ++q) {
        std::ofstream f(path(s, q), std::ios::binary | std::ios::trunc);
        if (!f) die("cannot create spill file " + path(s, q) + " (--spill-dir)");
      }
  }
  void flush(int set, int part) {
    std::string& b = pending[(size_t)set * parts + part];
    if (b.empty()) return;
    std::ofstream f(path(set, part), std::ios::binary | std::ios::app);
    f.write(b.data(), (std::streamsize)b.size());
    if (!f) die("write to spill file " + path(set, part) + " failed");
    bytes += (int64_t)b.size();
    b.clear();
  }
  void add(int set, const Variant& v) {
    const int part = (int)(std::hash<std::string>()(v.key) % (size_t)parts);
    std::string& b = pending[(size_t)set * parts + part];
    const uint32_t kl = (uint32_t)v.key.size(), nc = (uint32_t)v.carriers.size();
    b.append(reinterpret_cast<const char*>(&kl), 4);
    b.append(v.key);
    b.append(reinterpret_cast<const char*>(&nc), 4);
    b.append(reinterpret_cast<const char*>(v.carriers.data()), (size_t)nc * 4);
    counts[(size_t)set * parts + part] += 1;
    if (b.size() >= ((size_t)1 << 20)) flush(set, part);
  }
  void flush_all() {
    for (int s = 0; s < sets; ++s)
      for (int q = 0; q < parts; ++q) flush(s, q);
  }
  std::vector<Variant> read(int set, int part) const {
    std::vector<Variant> out;
    std::ifstream f(path(set, part), std::ios::binary | std::ios::ate);
    if (!f) die("cannot read spill file " + path(set, part));
    const std::streamsize size = f.tellg();
    f.seekg(0);
    std::string buf((size_t)size, '\0');
    f.read(&buf[0], size);
    size_t at = 0;
    out.reserve((size_t)counts[(size_t)set * parts + part]);
    while (at + 8 <= buf.size()) {
      uint32_t kl, nc;
      std::memcpy(&kl, &buf[at], 4);
      Variant v;
      v.key.assign(&buf[at + 4], kl);
      std::memcpy(&nc, &buf[at + 4 + kl], 4);
      v.carriers.resize(nc);
      if (nc) std::memcpy(v.carriers.data(), &buf[at + 8 + kl], (size_t)nc * 4);
      at += 8 + (size_t)kl + (size_t)nc * 4;
      out.push_back(std::move(v));
    }
    return out;
  }
  void remove_all() {
    for (int s = 0; s < sets; ++s)
      for (int q = 0; q < parts; ++q) (void)::unlink(path(s, q).c_str());
    sets = 0;
  }
  ~JoinSpill() { if (sets > 0) remove_all(); }
};

// getCallsRdd (:153-168) for two (joinDatasets :115-128) or more (mergeDatasets :130-148) sets of one key partition
void join_or_merge(const std::vector<std::vector<Variant>>& sets, std::vector<std::vector<int32_t>>& callsets) {
  if (sets.size() == 1) {   // one variant set: getCallsRdd takes its records as they are (:153-157)
    for (const auto& v : sets[0]) callsets.push_back(v.carriers);
  } else if (sets.size() == 2) {
    std::unordered_map<std::string, std::vector<const Variant*>> right;
    for (const auto& v : sets[1]) right[v.key].push_back(&v);
    for (const auto& v : sets[0]) {
      auto it = right.find(v.key);
      if (it == right.end()) continue;
      for (const Variant* w : it->second) {
        std::vector<int32_t> joined = v.carriers;
        joined.insert(joined.end(), w->carriers.begin(), w->carriers.end());
        callsets.push_back(std::move(joined));
      }
    }
  } else {
    std::map<std::string, std::vector<const Variant*>> groups;
    for (const auto& d : sets)
      for (const auto& v : d) groups[v.key].push_back(&v);
    for (const auto& g : groups) {
      if (g.second.size() != sets.size()) continue;
      std::vector<int32_t> merged;
      for (const Variant* v : g.second) merged.insert(merged.end(), v->carriers.begin(), v->carriers.end());
      callsets.push_back(std::move(merged));
    }
  }
}

struct CarrierFeeder {
  static constexpr int64_t kChunkRows = 1 << 16;
  unsigned char* pin[2] = {nullptr, nullptr};
  size_t pin_bytes = 0;
  int64_t rows_as_bits = 0, rows_as_lists = 0;
  ~CarrierFeeder() {
    for (unsigned char* b : pin)
      if (b) (void)pcoa_host_free_pinned(b);
  }
  // packs rows [r0, r1) (offsets relative to idx) into dst [rows][words]; returns false if some list repeats a callset
  static bool pack(const int32_t* idx, const int64_t* offs, int64_t r0, int64_t r1, int n, int64_t words, uint32_t* dst, unsigned threads) {
    std::atomic<bool> ok{true};
    const int64_t rows = r1 - r0;
    threads = (unsigned)std::max<int64_t>(1, std::min<int64_t>(threads, rows / 2048 + 1));
    auto work = [&](unsigned t) {
      const int64_t a = r0 + rows * t / threads, b = r0 + rows * (t + 1) / threads;
      for (int64_t r = a; r < b; ++r) {
        uint32_t* row = dst + (r - r0) * words;
        std::memset(row, 0, (size_t)words * 4);
        for (int64_t e = offs[r]; e < offs[r + 1]; ++e) {
          const int32_t c = idx[e];
          if (c < 0 || c >= n) die("callset index outside [0, N) in a carrier list");   // mapping(call.callsetId) throws (:59)
          uint32_t& w = row[c >> 5];
          if (w & (1u << (c & 31))) ok.store(false, std::memory_order_relaxed);
          w |= 1u << (c & 31);
        }
      }
    };
    if (threads == 1) work(0);
    else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < threads; ++t) th.emplace_back(work, t);
      for (auto& x : th) x.join();
    }
    return ok.load();
  }
  // idx / offs: CSR of `rows` carrier lists (offs[0] may be > 0: entries are idx[offs[r]] ..)
  void feed(pcoa_ctx* ctx, const Conf& conf, int n, const int32_t* idx, const int64_t* offs, int64_t rows, unsigned threads) {
    if (rows <= 0) return;
    const int64_t words = ((int64_t)n + 31) / 32;
    const int64_t nnz = offs[rows] - offs[0];
    const bool dense = conf.carrier_format == "bits" || (conf.carrier_format == "auto" && nnz > rows * words);
    auto as_lists = [&](int64_t r0, int64_t r1) {
      check(ctx, pcoa_accumulate_calls_ex(ctx, idx, offs + r0, r1 - r0, 0), "getSimilarityMatrix");
      rows_as_lists += r1 - r0;
    };
    if (!dense) {
      as_lists(0, rows);
      return;
    }
    const size_t need = (size_t)std::min(rows, kChunkRows) * (size_t)words * 4;
    if (need > pin_bytes) {
      for (unsigned char*& b : pin) {
        if (b) (void)pcoa_host_free_pinned(b);
        b = nullptr;
        void* q = nullptr;
        if (pcoa_host_alloc_pinned((size_t)kChunkRows * (size_t)words * 4, &q) != PCOA_OK) die("pcoa_host_alloc_pinned failed");
        b = static_cast<unsigned char*>(q);
      }
      pin_bytes = (size_t)kChunkRows * (size_t)words * 4;
    }
    // chunk k + 1 is packed (by `threads` threads, started from a helper thread) while chunk k is handed over
    int64_t r0 = 0;
    int k = 0;
    bool ok_cur = pack(idx, offs, 0, std::min(rows, kChunkRows), n, words, reinterpret_cast<uint32_t*>(pin[0]), threads);
    while (r0 < rows) {
      const int64_t r1 = std::min(rows, r0 + kChunkRows), r2 = std::min(rows, r1 + kChunkRows);
      bool ok_next = true;
      std::thread packer;
      if (r1 < rows)
        packer = std::thread([&, r1, r2, k] { ok_next = pack(idx, offs, r1, r2, n, words, reinterpret_cast<uint32_t*>(pin[(k + 1) & 1]), threads > 1 ? threads - 1 : 1); });
      if (!ok_cur && g_ld.on)
        die("--ld-window: a carrier list names a callset twice; a carrier bitset cannot carry that multiplicity");
      if (!ok_cur && conf.gram == "implicit")
        die("--gram implicit: a carrier list names a callset twice (a merge of sets with a repeated key); a carrier bitset cannot "
            "carry that multiplicity -- use --gram stored");
      if (ok_cur) {
        if (g_ld.on) g_ld.bits(ctx, reinterpret_cast<const uint32_t*>(pin[k & 1]), r1 - r0, words);
        else check(ctx, pcoa_accumulate_bits(ctx, reinterpret_cast<const uint32_t*>(pin[k & 1]), r1 - r0, words, 0), "getSimilarityMatrix");
        rows_as_bits += r1 - r0;
      } else {
        as_lists(r0, r1);
      }
      if (packer.joinable()) packer.join();
      ok_cur = ok_next;
      r0 = r1;
      ++k;
    }
  }
};

void stream_plink_shard(const Conf& conf, const PlinkMeta& m, int g, int k, pcoa_ctx* ctx, StreamStats* st,
                        unsigned char* const (&buf)[4]) {
  int64_t r0, r1;
  shard_range(g, k, (int64_t)m.keep.size(), &r0, &r1);
  const int fd = ::open((m.prefix + ".bed").c_str(), O_RDONLY);
  if (fd < 0) die("cannot open " + m.prefix + ".bed");
  const int64_t block = conf.stream_rows;
  const size_t bpv = m.bpv, words = (m.n + 31) / 32;
  const bool ref_a1 = conf.plink_ref_allele == "a1";
  // buf: four page-locked blocks of --stream-rows rows (pcoa_host_alloc_pinned): the engine's DMA reads them at link speed
  const unsigned read_threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency() / (2u * (unsigned)k)));
  ReaderPool pool(read_threads > 1 ? read_threads : 0);
  std::vector<uint32_t> bits;
  if (conf.plink_decode == "host") bits.resize((size_t)block * words);
  auto read_block = [&](int64_t b0, int which) -> int64_t {  // returns kept rows, compacted to the front of buf[which]
    const int64_t rows = std::min(block, r1 - b0);
    const size_t want = (size_t)rows * bpv;
    auto read_range = [&](size_t lo, size_t hi) {  // (one pread stream copies out of the page cache at ~6 GB/s: a few side by side)
      while (lo < hi) {
        const ssize_t r = ::pread(fd, buf[which] + lo, hi - lo, (off_t)(3 + (size_t)b0 * bpv + lo));
        if (r <= 0) die(m.prefix + ".bed: read error");
        lo += (size_t)r;
      }
    };
    if (read_threads <= 1 || want < ((size_t)8 << 20)) {
      read_range(0, want);
    } else {
      const size_t per = (want + read_threads - 1) / read_threads;
      pool.run([&](unsigned t) {
        const size_t lo = std::min(want, per * t), hi = std::min(want, per * (t + 1));
        if (hi > lo) read_range(lo, hi);
      });
    }
    int64_t kept = 0;
    for (int64_t r = 0; r < rows; ++r) {
      if (!m.keep[(size_t)(b0 + r)]) continue;
      if (kept != r) std::memmove(buf[which] + (size_t)kept * bpv, buf[which] + (size_t)r * bpv, bpv);
      ++kept;
    }
    return kept;
  };
  double read_s = 0, feed_s = 0;
  int64_t total = 0;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
  if (conf.plink_decode != "host") {
    // Device decode (r05): the feed call only QUEUES a block (PCOA_BED_HOST_ASYNC); a reader thread fills the next blocks
    // meanwhile.  Four blocks rotate: one being read, one filled and waiting, and the two the engine may still be copying
    // (pcoa.h: the rows of a queued call stay untouched until the second later call has returned).  The link idles only
    // while the reads are slower than the copies.
    constexpr int NB = 4;
    std::mutex mu;
    std::condition_variable cv;
    bool is_free[NB] = {true, true, true, true};
    std::deque<std::pair<int, int64_t>> filled;   // (block buffer, kept rows) in file order
    std::deque<int> queued;                       // buffers handed over, in call order
    bool reader_done = false;
    // (the reader takes ANY free buffer: tying block i to buffer i % 4 deadlocks when --references drops whole blocks --
    // no call is made for them, so the buffer the reader is waiting for is never released)
    std::thread reader([&] {
      for (int64_t b0 = r0; b0 < r1; b0 += block) {
        int w = -1;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] {
            for (int q = 0; q < NB; ++q)
              if (is_free[q]) {
                w = q;
                return true;
              }
            return false;
          });
          is_free[w] = false;
        }
        auto t0 = now();
        const int64_t kept = read_block(b0, w);
        read_s += secs(t0, now());
        {
          std::lock_guard<std::mutex> lk(mu);
          filled.emplace_back(w, kept);
        }
        cv.notify_all();
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        reader_done = true;
      }
      cv.notify_all();
    });
    for (;;) {
      int w = -1;
      int64_t kept = 0;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !filled.empty() || reader_done; });
        if (filled.empty()) break;
        w = filled.front().first;
        kept = filled.front().second;
        filled.pop_front();
      }
      auto t1 = now();
      if (kept > 0) {
        if (g_ld.on) g_ld.bed(ctx, buf[w], kept, (int64_t)bpv, ref_a1 ? 1 : 0);   // (synchronous: the rows are consumed when it returns)
        else if (g_calls.on)
          check(ctx, pcoa_accumulate_plink_bed_calls(ctx, g_calls.companion, buf[w], kept, (int64_t)bpv, ref_a1 ? 1 : 0, PCOA_BED_HOST_ASYNC),
                "getSimilarityMatrix");
        else check(ctx, pcoa_accumulate_plink_bed(ctx, buf[w], kept, (int64_t)bpv, ref_a1 ? 1 : 0, PCOA_BED_HOST_ASYNC), "getSimilarityMatrix");
        if (g_king.on)   // the same block to the five planes: it crosses the link a second time, through planes[0]'s staging slots
          check(g_king.planes[0], pcoa_accumulate_plink_bed_king(g_king.planes, buf[w], kept, (int64_t)bpv, PCOA_BED_HOST_ASYNC),
                "getSimilarityMatrix");
        total += kept;
      }
      feed_s += secs(t1, now());
      {
        std::lock_guard<std::mutex> lk(mu);
        if (kept <= 0) {
          is_free[w] = true;                              // nothing was handed over
        } else {
          queued.push_back(w);
          if (queued.size() > 2) {                        // two later CALLS have returned: that block is the reader's again
            is_free[queued.front()] = true;
            queued.pop_front();
          }
        }
      }
      cv.notify_all();
    }
    reader.join();
    auto t3 = now();
    check(ctx, pcoa_sync(ctx), "getSimilarityMatrix");  // the blocks are released by the caller next
    if (g_calls.on) check(g_calls.companion, pcoa_sync(g_calls.companion), "getSimilarityMatrix");
    if (g_king.on)
      for (pcoa_ctx* p : g_king.planes) check(p, pcoa_sync(p), "getSimilarityMatrix");
    feed_s += secs(t3, now());
  } else {
  int which = 0;
  std::future<int64_t> next;
  auto t0 = now();
  int64_t kept = r0 < r1 ? read_block(r0, 0) : 0;
  read_s += secs(t0, now());
  for (int64_t b0 = r0; b0 < r1; b0 += block) {
    const int64_t b1 = b0 + block;
    if (b1 < r1) next = std::async(std::launch::async, read_block, b1, which ^ 1);  // the next block is read beside this one's feed
    auto t1 = now();
    if (kept > 0) {
      const unsigned nt = std::max(1u, std::min<unsigned>(conf.ingest_threads > 0 ? (unsigned)conf.ingest_threads : std::thread::hardware_concurrency(), 16u) / (unsigned)k);
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
          for (int64_t r = t; r < kept; r += nt)
            bed_row_to_bits(buf[which] + (size_t)r * bpv, bpv, m.n, ref_a1, bits.data() + (size_t)r * words, words);
        });
      for (auto& x : th) x.join();
      if (g_ld.on) g_ld.bits(ctx, bits.data(), kept, (int64_t)words);
      else check(ctx, pcoa_accumulate_bits(ctx, bits.data(), kept, (int64_t)words, 0), "getSimilarityMatrix");
      total += kept;
    }
    feed_s += secs(t1, now());
    if (b1 < r1) {
      auto t2 = now();
      kept = next.get();
      read_s += secs(t2, now());  // (only what the feed did not hide)
      which ^= 1;
    }
  }
  }
  ::close(fd);
  std::lock_guard<std::mutex> lk(st->mu);
  st->variants += total;
  st->read_s = std::max(st->read_s, read_s);
  st->feed_s = std::max(st->feed_s, feed_s);
}

// --project-input-path: every joined row goes to BOTH engines as one carrier bitset of all N samples, packed once -- the
// reference engine (N_ref samples) ignores the bits of samples >= N_ref (pcoa_accumulate_bits), the strip owner over columns
// [N_ref, N) takes them all.  A row that names a callset twice cannot be a bitset: refused.
struct ProjectionFeeder {
  pcoa_ctx* ref = nullptr;
  pcoa_ctx* cross = nullptr;
  uint32_t* pin = nullptr;
  int64_t rows_fed = 0;
  ~ProjectionFeeder() { if (pin) (void)pcoa_host_free_pinned(pin); }
  void feed(int n, const int32_t* idx, const int64_t* offs, int64_t rows, unsigned threads) {
    const int64_t words = ((int64_t)n + 31) / 32;
    if (!pin) {
      void* q = nullptr;
      if (pcoa_host_alloc_pinned((size_t)CarrierFeeder::kChunkRows * (size_t)words * 4, &q) != PCOA_OK) die("pcoa_host_alloc_pinned failed");
      pin = static_cast<uint32_t*>(q);
    }
    for (int64_t r0 = 0; r0 < rows; r0 += CarrierFeeder::kChunkRows) {
      const int64_t r1 = std::min(rows, r0 + CarrierFeeder::kChunkRows);
      if (!CarrierFeeder::pack(idx, offs, r0, r1, n, words, pin, threads))
        die("--project-input-path: a joined variant names a callset twice; a carrier bitset cannot carry that multiplicity");
      check(ref, pcoa_accumulate_bits(ref, pin, r1 - r0, words, 0), "getSimilarityMatrix (reference)");
      check(cross, pcoa_accumulate_bits(cross, pin, r1 - r0, words, 0), "getSimilarityMatrix (projected samples)");
    }
    rows_fed += rows;
  }
};

// --project-input-path: what cannot be served is refused before any file is read or any device is touched
void check_projection_conf(const Conf& conf) {
  if (conf.project_input_path.empty()) return;
  if (conf.gpus > 1) die("--project-input-path runs on one GPU: it cannot take --gpus " + std::to_string(conf.gpus));
  if (conf.layout == "strips") die("--project-input-path needs the reference's S whole on one engine: it cannot take --layout strips");
  if (conf.carrier_format == "lists") die("--project-input-path feeds both engines carrier bitsets: it cannot take --carrier-format lists");
  std::set<std::string> stems;
  auto stem_of = [](const std::string& path) {
    std::string stem = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
    stem = stem.substr(0, stem.find('.'));
    std::replace(stem.begin(), stem.end(), '-', '_');
    return stem;
  };
  for (const auto& p : conf.input_path) {
    if (is_plink_path(p)) die("--project-input-path needs VCF inputs on both sides: " + p + " is a PLINK fileset");
    stems.insert(stem_of(p));
  }
  for (const auto& p : conf.project_input_path) {
    if (is_plink_path(p)) die("--project-input-path needs VCF inputs on both sides: " + p + " is a PLINK fileset");
    const std::string st = stem_of(p);
    if (!stems.insert(st).second)
      die("--project-input-path: callset-id collision: " + p + " has the set id '" + st + "' of an earlier input (callset ids are "
          "<set id>-<column>); rename the file");
  }
}

// k engines, fed by k host threads, reduced into engine 0 (VariantsPca.scala:190: reduceByKey).  RCCL where every engine has
// a device of its own and the collective runtime binds; else peer copies + int64 adds (pcoa_gram_reduce_from), which also work
// with several engines on ONE device (--gpu-map 0,0: the way this path is tested on a single-GPU box).
//
// The strip layout (`strips`: one column range per engine) has no reduction: engine g is a strip owner of
// S[:, col0_g .. col0_g + cols_g) and is fed EVERY variant -- feed(g, 0, 1, ..): its thread runs the whole ingest road --,
// and all k owners come back.  Otherwise feed(g, g, k, ..) gives engine g its shard and only engine 0 comes back.
std::vector<pcoa_ctx*> run_engines(const Conf& conf, int32_t n, const std::vector<std::pair<int32_t, int32_t>>& strips,
                                   const std::function<void(int, int, int, pcoa_ctx*)>& feed, std::string* how,
                                   double* feed_seconds, const std::function<void(const std::vector<pcoa_ctx*>&)>& prepare) {
  const int k = conf.gpus;
  const bool tiled = !strips.empty();
  std::vector<pcoa_ctx*> ctx((size_t)k, nullptr);
  for (int g = 0; g < k; ++g) {
    const bool op = conf.gram == "implicit";
    const int rc = tiled ? pcoa_create_strip(&ctx[(size_t)g], n, strips[(size_t)g].first, strips[(size_t)g].second,
                                             conf.gpu_map[(size_t)g], PCOA_FLAG_DEFAULT)
                   : conf.grm ? pcoa_create_grm(&ctx[(size_t)g], n, conf.gpu_map[(size_t)g], PCOA_FLAG_DEFAULT)
                   : op  ? pcoa_create_operator(&ctx[(size_t)g], n, conf.gpu_map[(size_t)g], PCOA_FLAG_DEFAULT)
                         : pcoa_create(&ctx[(size_t)g], n, conf.gpu_map[(size_t)g], PCOA_FLAG_DEFAULT);
    if (rc != PCOA_OK)
      die(std::string(tiled ? "pcoa_create_strip" : conf.grm ? "pcoa_create_grm" : op ? "pcoa_create_operator" : "pcoa_create") + " on device " + std::to_string(conf.gpu_map[(size_t)g]) +
          ": " + pcoa_last_error(nullptr));
  }
  // operand buffers and the computePca workspace now, not inside the first accumulate calls (pcoa_reserve: the warm-up a Spark
  // executor runs once per GPU)
  for (int g = 0; g < k; ++g) check(ctx[(size_t)g], pcoa_reserve(ctx[(size_t)g], (int64_t)1 << 20, g == 0 ? conf.num_pc : 0), "pcoa_reserve");
  bool distinct = true;
  for (int a = 0; a < k; ++a)
    for (int b = a + 1; b < k; ++b) distinct = distinct && conf.gpu_map[(size_t)a] != conf.gpu_map[(size_t)b];
  bool use_rccl = !tiled && k > 1 && (conf.reduce == "rccl" || (conf.reduce == "auto" && distinct));
  if (use_rccl && !distinct) die("--reduce rccl needs a device of its own for every engine");
  uint8_t uid[128] = {0};
  if (use_rccl && pcoa_comm_unique_id(uid) != PCOA_OK) {
    if (conf.reduce == "rccl") die("pcoa_comm_unique_id failed: no collective runtime");
    use_rccl = false;  // auto: no RCCL to bind -> peer reduction
  }
  std::vector<int> rccl_rc((size_t)k, PCOA_OK);
  std::vector<std::thread> th;
  prepare(ctx);  // (what the feed needs once a HIP device is up: the pinned blocks of the streaming reader, their first use)
  const auto t_feed = std::chrono::steady_clock::now();  // engines exist: from here to the reduced S is the job
  for (int g = 0; g < k; ++g)
    th.emplace_back([&, g] {
      feed(g, tiled ? 0 : g, tiled ? 1 : k, ctx[(size_t)g]);
      if (use_rccl) {  // every rank reaches the collective from its own thread
        void* comm = nullptr;
        int rc = pcoa_comm_init(ctx[(size_t)g], uid, g, k, &comm);
        if (rc == PCOA_OK) rc = pcoa_gram_allreduce_rccl(ctx[(size_t)g], comm);
        if (comm) (void)pcoa_comm_destroy(comm);
        rccl_rc[(size_t)g] = rc;
      }
    });
  for (auto& t : th) t.join();
  if (use_rccl) {
    for (int g = 0; g < k; ++g)
      if (rccl_rc[(size_t)g] != PCOA_OK) die(std::string("all-reduce over RCCL: ") + pcoa_last_error(ctx[(size_t)g]));
    *how = "RCCL all-reduce over " + std::to_string(k) + " engines";
  } else if (tiled) {
    *how = "strip layout: " + std::to_string(k) + " owner(s), each fed every variant, no reduction; columns";
    for (int g = 0; g < k; ++g)
      *how += (g ? ", [" : " [") + std::to_string(strips[(size_t)g].first) + ", " +
              std::to_string(strips[(size_t)g].first + strips[(size_t)g].second) + ") on device " +
              std::to_string(conf.gpu_map[(size_t)g]);
  } else if (k > 1) {
    // --reduce scatter: all k engines at once, 1 / k of S per link, nothing staged.  Engines that cannot address each other's
    // memory are the one case the library hands back (PCOA_ERR_STATE): the chain below then does the job
    bool scattered = false;
    if (conf.reduce == "scatter") {
      const int rc = pcoa_gram_reduce_peers(ctx.data(), k, 1);
      if (rc == PCOA_ERR_STATE) std::fprintf(stderr, "%s; falling back to the peer reduction into engine 0\n", pcoa_last_error(ctx[0]));
      else check(ctx[0], rc, "reduce");
      scattered = rc == PCOA_OK;
    }
    if (scattered) {
      *how = "reduce-scatter over " + std::to_string(k) + " engines, total gathered on engine 0";
    } else {
      for (int g = 1; g < k; ++g) check(ctx[0], pcoa_gram_reduce_from(ctx[0], ctx[(size_t)g]), "reduce");
      *how = "peer reduction of " + std::to_string(k) + " engines into engine 0";
    }
  } else {
    *how = conf.grm ? "one GRM engine: the 2-bit genotypes kept, no matrix"
           : conf.gram == "implicit" ? "one operator engine: the carrier bitsets kept, no similarity matrix" : "one engine";
  }
  for (int g = 0; g < (tiled ? k : 1); ++g) check(ctx[(size_t)g], pcoa_gram_finalize(ctx[(size_t)g]), "getSimilarityMatrix");
  *feed_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_feed).count();
  if (tiled) return ctx;
  for (int g = 1; g < k; ++g) pcoa_destroy(ctx[(size_t)g]);
  return {ctx[0]};
}

// emitResult (:233-246): name, dataset, pc1, pc2 sorted by name on stdout (+ <output-path>-pca.tsv)
struct OutRow { std::string name, dataset; double pc1, pc2; };
// n_study (--grm-project-path): the last n_study rows are the projected samples: they follow the panel's, sorted among themselves
void emit_result(const Conf& conf, std::vector<OutRow>& rows, size_t n_study = 0) {
  const auto by_name = [](const OutRow& a, const OutRow& b) { return a.name < b.name; };
  std::stable_sort(rows.begin(), rows.end() - (std::ptrdiff_t)n_study, by_name);
  std::stable_sort(rows.end() - (std::ptrdiff_t)n_study, rows.end(), by_name);
  for (const auto& r : rows)
    std::printf("%s\t%s\t%s\t%s\n", r.name.c_str(), r.dataset.c_str(), java_double(r.pc1).c_str(), java_double(r.pc2).c_str());
  if (!conf.output_path.empty()) {
    std::string target = conf.output_path + "-pca.tsv";
    if (conf.spark_output) {   // what resultRDD.saveAsTextFile(outputPath) leaves (:241-245): a directory; like Spark, an existing one is an error
      if (::mkdir(target.c_str(), 0777) != 0) die("output directory " + target + " already exists (or cannot be created)");
      std::ofstream(target + "/_SUCCESS");
      target += "/part-00000";
    }
    std::ofstream out(target);
    for (const auto& r : rows)
      out << r.name << "\t" << java_double(r.pc1) << "\t" << java_double(r.pc2) << "\t" << r.dataset << "\n";
  }
}

// The outlier rule of --outlier-iterations, as variants_pca.py's outlier_rule states it: comps is [num_pc][n].  Per axis:
// mean = (sum of the n entries) / n, sd = sqrt((sum of the squared deviations from the mean) / n) -- the population standard
// deviation --, both sums added left to right in double; sample i is removed if |u[i] - mean| > sigma * sd on any axis with
// sd > 0.
std::vector<char> outlier_rule(const double* comps, int num_pc, int32_t n, double sigma) {
  std::vector<char> removed((size_t)n, 0);
  for (int c = 0; c < num_pc; ++c) {
    const double* u = comps + (size_t)c * (size_t)n;
    double sum = 0.0;
    for (int32_t i = 0; i < n; ++i) sum += u[i];
    const double mean = sum / n;
    double ss = 0.0;
    for (int32_t i = 0; i < n; ++i) {
      const double d = u[i] - mean;
      ss += d * d;
    }
    const double sd = std::sqrt(ss / n);
    if (!(sd > 0)) continue;
    for (int32_t i = 0; i < n; ++i)
      if (std::fabs(u[i] - mean) > sigma * sd) removed[(size_t)i] = 1;
  }
  return removed;
}

// The removal rule of --remove-related, as variants_pca.py's related_removal states it: while any reported pair has both
// samples still kept, the kept sample with the most kept partners is removed; a tie goes to the highest index; the partners'
// counts are updated and the step repeats.  Returns the removed samples in increasing order.
std::vector<int32_t> related_removal(const std::vector<pcoa_pair>& pairs, int32_t n) {
  std::vector<std::vector<int32_t>> partners((size_t)n);
  for (const pcoa_pair& p : pairs) {
    partners[(size_t)p.i].push_back(p.j);
    partners[(size_t)p.j].push_back(p.i);
  }
  std::vector<int64_t> degree((size_t)n);
  for (int32_t i = 0; i < n; ++i) degree[(size_t)i] = (int64_t)partners[(size_t)i].size();   // (the library reports a pair once)
  std::vector<char> gone((size_t)n, 0);
  std::vector<int32_t> removed;
  for (;;) {
    int32_t v = -1;
    int64_t most = 0;
    for (int32_t i = 0; i < n; ++i)
      if (degree[(size_t)i] > 0 && degree[(size_t)i] >= most) { most = degree[(size_t)i]; v = i; }
    if (v < 0) break;
    removed.push_back(v);
    gone[(size_t)v] = 1;
    for (int32_t w : partners[(size_t)v])
      if (!gone[(size_t)w]) --degree[(size_t)w];
    degree[(size_t)v] = 0;
  }
  std::sort(removed.begin(), removed.end());
  return removed;
}

// --grm-project-path, before any engine exists: the study is a PLINK fileset whose .bim equals the panel's line by line in contig,
// id, position and both alleles (a fileset with the alleles exchanged is refused, not flipped), and none of its sample names
// repeats a panel name
void check_grm_study(const std::string& panel_path, const std::string& study_path) {
  if (!is_plink_path(study_path)) die("--grm --grm-project-path must name a PLINK .bed / .bim / .fam, not " + study_path);
  const std::string panel = panel_path.substr(0, panel_path.size() - 4), study = study_path.substr(0, study_path.size() - 4);
  auto fields = [](const std::string& file) {
    std::ifstream in(file);
    if (!in) die("cannot open " + file);
    std::vector<std::vector<std::string>> out;
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream is(line);
      std::vector<std::string> t;
      std::string w;
      while (is >> w) t.push_back(w);
      if (!t.empty()) out.push_back(t);
    }
    return out;
  };
  const auto a = fields(panel + ".bim"), b = fields(study + ".bim");
  const std::string head = "--grm --grm-project-path: " + study + ".bim and " + panel + ".bim differ at line ";
  for (size_t k = 0; k < std::max(a.size(), b.size()); ++k) {
    if (k >= a.size() || k >= b.size())
      die(head + std::to_string(k + 1) + ": " + (k >= b.size() ? study : panel) + ".bim ends after " +
          std::to_string(std::min(a.size(), b.size())) + " lines (both filesets must hold the same variants in the same order)");
    const auto& x = a[k];
    const auto& y = b[k];
    if (x.size() < 6 || y.size() < 6) die(head + std::to_string(k + 1) + ": a .bim line has six columns");
    const bool same3 = x[0] == y[0] && x[1] == y[1] && x[3] == y[3];
    if (same3 && x[4] == y[4] && x[5] == y[5]) continue;
    const bool swapped = same3 && x[4] == y[5] && x[5] == y[4];
    die(head + std::to_string(k + 1) + ": study '" + y[0] + " " + y[1] + " " + y[3] + " " + y[4] + " " + y[5] + "', panel '" + x[0] + " " +
        x[1] + " " + x[3] + " " + x[4] + " " + x[5] + "'" + (swapped ? ": the alleles are exchanged, and genotypes are not flipped" : "") +
        " (contig, id, position and both alleles must agree)");
  }
  std::set<std::string> seen;
  for (const auto& t : fields(panel + ".fam"))
    if (t.size() >= 2) seen.insert(t[1]);
  for (const auto& t : fields(study + ".fam"))
    if (t.size() >= 2 && seen.count(t[1]))
      die("--grm --grm-project-path: the study sample '" + t[1] + "' of " + study + ".fam repeats a sample name of the panel");
}

// --grm-keep-samples / --grm-remove-samples, before any engine exists: names are the fileset's sample names in index order.
// Returns false without a list, else *kept = the kept indices, increasing.  An unknown or repeated name is refused.
bool grm_sample_list(const Conf& conf, const std::vector<std::string>& names, std::vector<int32_t>* kept) {
  const bool keeping = !conf.grm_keep_samples.empty();
  const std::string flag = keeping ? "--grm-keep-samples" : "--grm-remove-samples";
  const std::string& path = keeping ? conf.grm_keep_samples : conf.grm_remove_samples;
  if (path.empty()) return false;
  std::unordered_map<std::string, int32_t> index;
  for (size_t i = 0; i < names.size(); ++i) index[names[i]] = (int32_t)i;
  std::ifstream in(path);
  if (!in) die(flag + ": cannot read " + path);
  std::vector<char> listed(names.size(), 0);
  std::string line;
  while (std::getline(in, line)) {
    const size_t a = line.find_first_not_of(" \t\r\n"), b = line.find_last_not_of(" \t\r\n");
    if (a == std::string::npos) continue;
    const std::string name = line.substr(a, b - a + 1);
    const auto it = index.find(name);
    if (it == index.end()) die("--grm " + flag + ": '" + name + "' of " + path + " is not a sample of the fileset");
    if (listed[(size_t)it->second]) die("--grm " + flag + ": '" + name + "' is listed twice in " + path);
    listed[(size_t)it->second] = 1;
  }
  kept->clear();
  for (size_t i = 0; i < names.size(); ++i)
    if ((listed[i] != 0) == keeping) kept->push_back((int32_t)i);
  const int32_t least = std::max(32, conf.num_pc + 1);
  if ((int32_t)kept->size() < least)
    die("--grm " + flag + " leaves " + std::to_string(kept->size()) + " of " + std::to_string(names.size()) + " samples, fewer than the " +
        std::to_string(least) + " a GRM engine with " + std::to_string(conf.num_pc) + " principal components needs");
  return true;
}

// The samples of `study` on the panel's axes -- mean-imputed (pcoa_grm_project), or with --grm-project-lsq by least squares
// (pcoa_grm_project_lsq) -- and the stderr line(s).  labels[q]: the name a message gives sample q.  coords: [num_pc][nq].  Returns
// placed [nq]: an undetermined sample of the least-squares form is named on stderr and not placed
std::vector<char> grm_place(const Conf& conf, pcoa_ctx* panel, pcoa_ctx* study, int32_t nq, const std::vector<double>& comps,
                            const std::vector<double>& lam, const char* what, const std::vector<std::string>& labels,
                            std::vector<double>& coords) {
  coords.assign((size_t)conf.num_pc * (size_t)nq, 0.0);
  std::vector<int32_t> called((size_t)nq), determined((size_t)nq, 1);
  if (conf.grm_project_lsq)
    check(panel, pcoa_grm_project_lsq(panel, study, conf.num_pc, comps.data(), coords.data(), called.data(), determined.data(), nullptr),
          "pcoa_grm_project_lsq");
  else
    check(panel, pcoa_grm_project(panel, study, conf.num_pc, comps.data(), lam.data(), coords.data(), called.data()), "pcoa_grm_project");
  int64_t used = 0, total_called = 0;
  if (pcoa_grm_info(panel, nullptr, &used, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(panel));
  for (int32_t c : called) total_called += c;
  const double share = (double)total_called / (double)nq / (double)used;
  std::vector<char> placed((size_t)nq, 1);
  if (!conf.grm_project_lsq) {
    std::fprintf(stderr, "Projected %d %ssamples over %lld used variants (mean call share %.4f)\n", nq, what, (long long)used, share);
    return placed;
  }
  int32_t undetermined = 0;
  for (int32_t q = 0; q < nq; ++q) undetermined += determined[(size_t)q] ? 0 : 1;
  std::fprintf(stderr, "Projected %d %ssamples over %lld used variants (mean call share %.4f, least squares, %d undetermined)\n", nq, what,
               (long long)used, share, undetermined);
  for (int32_t q = 0; q < nq; ++q) {
    if (determined[(size_t)q]) continue;
    placed[(size_t)q] = 0;
    std::fprintf(stderr, "Not placed: %s is called at %d of %lld used variants, which do not determine %d coordinates\n",
                 labels[(size_t)q].c_str(), called[(size_t)q], (long long)used, conf.num_pc);
  }
  return placed;
}

// --grm-project-path: the study's kept .bed rows into a GRM study store, block by block, and its samples onto the panel's axes.
// comps / lam: what pcoa_compute returned on the panel.  Returns the study's rows in .fam order; *called_share: the mean over
// the samples of (used variants at which the sample is called) / (used variants)
std::vector<OutRow> grm_project_study(const Conf& conf, pcoa_ctx* panel, const PlinkMeta& panel_meta, const std::vector<double>& comps,
                                      const std::vector<double>& lam, std::set<std::string>& used_stems) {
  const PlinkMeta sm = read_plink_meta(conf.grm_project_path, set_id_of(conf.grm_project_path, 1, used_stems), {});
  if (sm.keep.size() != panel_meta.keep.size()) die("--grm-project-path: the study's .bim changed while the job ran");
  const int32_t nq = (int32_t)sm.n;
  pcoa_ctx* study = nullptr;
  if (pcoa_create_grm_study(&study, nq, conf.gpu_map[0], PCOA_FLAG_DEFAULT) != PCOA_OK)
    die(std::string("pcoa_create_grm_study: ") + pcoa_last_error(nullptr));
  {
    std::ifstream bed(sm.prefix + ".bed", std::ios::binary);
    bed.seekg(3);
    const size_t bpv = sm.bpv, total = sm.keep.size(), block = (size_t)conf.stream_rows;
    std::vector<unsigned char> buf(std::min(block, std::max<size_t>(total, 1)) * bpv);
    for (size_t b0 = 0; b0 < total; b0 += block) {
      const size_t nrows = std::min(block, total - b0);
      bed.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(nrows * bpv));
      if ((size_t)bed.gcount() != nrows * bpv) die(sm.prefix + ".bed: read error");
      size_t kept_rows = 0;
      for (size_t r = 0; r < nrows; ++r) {
        if (!panel_meta.keep[b0 + r]) continue;   // (the panel's mask: the .bim files are equal)
        if (kept_rows != r) std::memmove(buf.data() + kept_rows * bpv, buf.data() + r * bpv, bpv);
        ++kept_rows;
      }
      if (kept_rows > 0)
        check(study, pcoa_accumulate_plink_bed(study, buf.data(), (int64_t)kept_rows, (int64_t)bpv, conf.plink_ref_allele == "a1" ? 1 : 0, 0),
              "pcoa_accumulate_plink_bed (study)");
    }
  }
  check(study, pcoa_gram_finalize(study), "pcoa_gram_finalize (study)");
  std::vector<double> coords;
  const std::vector<char> placed = grm_place(conf, panel, study, nq, comps, lam, "", sm.names, coords);
  pcoa_destroy(study);
  std::vector<OutRow> rows;
  for (int32_t q = 0; q < nq; ++q)
    if (placed[(size_t)q])
      rows.push_back({sm.names[(size_t)q], sm.ids[(size_t)q].substr(0, sm.ids[(size_t)q].find('-')), coords[(size_t)q],
                    coords[(size_t)q + (size_t)nq]});
  return rows;
}

int main(int argc, char** argv) {
  const auto t_start = std::chrono::steady_clock::now();
  Conf conf = parse(argc, argv);
  if (conf.grm && !conf.grm_project_path.empty()) check_grm_study(conf.input_path[0], conf.grm_project_path);
  const bool want_loadings = !conf.loadings_output_path.empty();
  g_ld.on = conf.ld_window > 0;
  g_calls.on = conf.missing_calls == "pairwise";
  g_king.on = conf.king;
  g_want_meta = want_loadings || g_ld.on || !conf.grm_weights_output_path.empty() || conf.grm_ld_window > 0 ||
                !conf.grm_variant_qc_output_path.empty();   // (--ld-window: the contigs place the breaks)
  if (conf.input_path.empty())
    die("--input-path <file.vcf[.gz]> [more files] or one PLINK fileset (<prefix>.bed) is required: the Google Genomics API the reference read "
        "from has been shut down");
  // --project-input-path: those sets follow the reference's, so their callsets take the indexes [N_ref, N) (the concatenation
  // rule below) and their variants are matched by the join / merge of all sets
  check_projection_conf(conf);
  const bool projecting = !conf.project_input_path.empty();
  const size_t n_ref_inputs = conf.input_path.size();
  conf.input_path.insert(conf.input_path.end(), conf.project_input_path.begin(), conf.project_input_path.end());
  int32_t n_ref = 0;
  // VariantsCommon (VariantsCommon.scala:33-66): callset index/name maps + one dataset per variant set
  std::vector<Dataset> data;
  std::vector<std::string> ids, names;
  std::set<std::string> used_stems;
  // A single PLINK fileset is STREAMED (r04): only the .fam and the .bim are read up front; the .bed goes through
  // stream_plink_shard block by block, each engine its own contiguous range of variants.
  const bool stream_plink = conf.input_path.size() == 1 && is_plink_path(conf.input_path[0]) && !conf.no_stream &&
                            !conf.parse_only && !conf.has_maf;
  if (want_loadings && conf.gram != "implicit" && !stream_plink)
    die("--loadings-output-path with a stored similarity matrix takes its second pass over ONE streamed PLINK fileset; for this "
        "input use --gram implicit, which keeps the rows resident");
  std::vector<VarMeta> fed_meta;   // --loadings-output-path: (contig, position, id) of every row fed, in feed order
  bool fed_meta_known = true;      // joined / merged sets reach the engine partition by partition without their records: '.' columns
  PlinkMeta plink;
  if (stream_plink) {
    std::vector<Region> regions;
    if (!conf.all_references && !conf.references.empty()) regions = parse_references(conf.references[0]);
    plink = read_plink_meta(conf.input_path[0], set_id_of(conf.input_path[0], 0, used_stems), regions);
    ids = plink.ids;
    names = plink.names;
  }
  std::vector<int32_t> grm_mind_gone;   // --grm-mind: the samples it took out (never placed by --grm-project-removed)
  std::vector<int32_t> grm_listed;   // --grm-keep-samples / --grm-remove-samples: the kept indices; a wrong list is refused here
  bool grm_has_list = conf.grm && grm_sample_list(conf, names, &grm_listed);   // (--grm-mind joins the list after the feed)
  const bool grm_rounds = conf.grm && (grm_has_list || conf.grm_outlier_iterations > 0 || conf.grm_cutoff_given || conf.grm_king || conf.has_grm_mind);
  // A single VCF is streamed as well (r05): the header gives the callsets, then every 16-MiB block is parsed by the thread
  // pool, filtered (--references, --min-allele-frequency) and handed to the engine as carrier lists while the next one is
  // read -- the records of the whole file are never held (VariantsRDD.compute is an iterator, rdd/VariantsRDD.scala:205-235).
  // Joins and merges need whole data sets, --gpus k a known row count: those keep the in-memory path.
  // The streaming path opens the input twice (header, then records): only a REGULAR file can be read twice -- a FIFO,
  // /dev/stdin or a process substitution is consumed by the first pass and takes the one-pass in-memory path.
  auto is_regular_file = [](const std::string& path) {
    struct stat sb;
    return ::stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode);
  };
  const bool stream_vcf = conf.input_path.size() == 1 && !is_plink_path(conf.input_path[0]) && !conf.no_stream &&
                          !conf.parse_only && !conf.debug_datasets && conf.gpus == 1 && is_regular_file(conf.input_path[0]);
  // Several VCFs (join / merge) are streamed too (r06): one pass per set into hash-partitioned spill files, then one key
  // partition at a time (JoinSpill above).  --debug-datasets prints per-record lines in file order and keeps the in-memory path.
  // A single VCF for SEVERAL engines (--gpus k) takes the same road with one set: the parser's one pass deals the records to
  // the key partitions, engine g feeds partitions g, g + k, .. -- the r05 path parsed the whole file into memory first.
  // (--parse-only takes the same road for two or more sets, so that the CPU test tier holds the spill + partition-wise join to
  // the in-memory path; a single VCF is parsed in memory there as before.)
  bool stream_join = ((conf.input_path.size() >= 2) || (conf.gpus > 1 && !conf.parse_only)) && !conf.no_stream && !conf.debug_datasets;
  for (const auto& pth : conf.input_path) stream_join = stream_join && !is_plink_path(pth) && is_regular_file(pth);
  JoinSpill spill;
  std::vector<std::string> join_stems;
  std::vector<std::vector<Region>> join_regions;
  std::vector<int32_t> join_base;
  std::string stream_stem;
  std::vector<Region> stream_regions;
  int64_t streamed_variants = 0;
  if (n_ref_inputs > 1) std::printf("Running PCA on %zu datasets.\n", n_ref_inputs);
  for (size_t k = 0; k < conf.input_path.size() && !stream_plink; ++k) {
    std::vector<Region> regions;
    if (!conf.all_references && !conf.references.empty())
      regions = parse_references(conf.references[std::min(k, conf.references.size() - 1)]);
    if (is_plink_path(conf.input_path[k])) {
      if (conf.input_path.size() > 1 || conf.has_maf)
        die("joining variant sets or filtering by allele frequency needs VCF inputs: a PLINK fileset is read as carriers "
            "only (no ref/alt keys, no INFO/AF)");
      data.push_back(load_plink(conf.input_path[k], set_id_of(conf.input_path[k], k, used_stems), regions, (int32_t)ids.size(),
                                conf.plink_ref_allele == "a1"));
    } else {
      const std::string stem = set_id_of(conf.input_path[k], k, used_stems);
      if (stream_vcf) {
        stream_stem = stem;
        stream_regions = regions;
      }
      if (stream_join) {
        join_stems.push_back(stem);
        join_regions.push_back(regions);
        join_base.push_back((int32_t)ids.size());
      }
      data.push_back(load_vcf(conf.input_path[k], stem, regions, (int32_t)ids.size(), conf.debug_datasets, conf.ingest_threads,
                              nullptr, stream_vcf || stream_join));
    }
    ids.insert(ids.end(), data.back().ids.begin(), data.back().ids.end());
    names.insert(names.end(), data.back().names.begin(), data.back().names.end());
    if (k + 1 == n_ref_inputs) n_ref = (int32_t)ids.size();
  }
  const int32_t n = (int32_t)ids.size();
  std::printf("Matrix size: %d.\n", projecting ? n_ref : n);
  if (n == 0) die("no samples");

  // streamed join / merge, pass 1: every set once through the parser threads into its key partitions' spill files
  int64_t spilled_records = 0;
  if (stream_join) {
    spill.open(conf, (int)conf.input_path.size());
    for (size_t k = 0; k < conf.input_path.size(); ++k) {
      if (conf.has_maf) std::printf("Min allele frequency %s.\n", java_number<float>(conf.min_allele_frequency).c_str());  // per dataset (:43)
      const std::function<void(std::vector<ParsedLine>&)> to_spill = [&](std::vector<ParsedLine>& parsed) {
        for (auto& pl : parsed) {
          if (!pl.keep) continue;
          if (conf.has_maf && !(pl.v.has_af && pl.v.af >= conf.min_allele_frequency)) continue;   // filterDataset (:96-108)
          spill.add((int)k, pl.v);
          spilled_records += 1;
        }
      };
      (void)load_vcf(conf.input_path[k], join_stems[k], join_regions[k], join_base[k], false, conf.ingest_threads, &to_spill);
    }
    spill.flush_all();
  }

  // filterDataset (:96-108)
  if (conf.has_maf && !stream_join) {
    for (auto& d : data) {
      std::printf("Min allele frequency %s.\n", java_number<float>(conf.min_allele_frequency).c_str());  // per dataset (:43)
      std::vector<Variant> kept;
      for (auto& v : d.variants)
        if (v.has_af && v.af >= conf.min_allele_frequency) kept.push_back(std::move(v));
      d.variants.swap(kept);
    }
  }

  // getCallsRdd (:153-168)
  std::vector<std::vector<int32_t>> callsets;
  if (data.size() == 1) {
    for (auto& v : data[0].variants) {
      if (g_want_meta && !v.carriers.empty() && !stream_vcf && !stream_join) fed_meta.push_back(v.meta);
      callsets.push_back(std::move(v.carriers));
    }
  } else if (!stream_join) {  // joinDatasets (two sets) / mergeDatasets (more)
    std::vector<std::vector<Variant>> sets;
    for (auto& d : data) sets.push_back(std::move(d.variants));
    join_or_merge(sets, callsets);
  } else if (conf.parse_only) {   // the streamed join without a GPU: every key partition in turn, rows collected for the report
    for (int q = 0; q < spill.parts; ++q) {
      std::vector<std::vector<Variant>> sets;
      for (int sset = 0; sset < spill.sets; ++sset) sets.push_back(spill.read(sset, q));
      join_or_merge(sets, callsets);
    }
    std::printf("Streamed join: %zu variant sets through %d key partitions, %lld records, %.1f MB of spill files.\n",
                conf.input_path.size(), spill.parts, (long long)spilled_records, spill.bytes / 1e6);
    spill.remove_all();
  }
  std::vector<int32_t> sample_idx;
  std::vector<int64_t> row_offsets{0};
  for (const auto& calls : callsets) {
    if (calls.empty()) continue;  // variants without a varying call are dropped (:166)
    sample_idx.insert(sample_idx.end(), calls.begin(), calls.end());
    row_offsets.push_back((int64_t)sample_idx.size());
  }
  if (conf.parse_only) {
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    std::printf("Variants with variation: %zu; carriers: %zu; ingest + getCallsRdd %.3f s (read %.3f, split %.3f, "
                "parse %.3f)\n", row_offsets.size() - 1, sample_idx.size(), secs, g_ingest_read_s, g_ingest_split_s,
                g_ingest_parse_s);
    if (!conf.output_path.empty()) {  // the RDD[Seq[Int]] of getCallsRdd, one variant per line
      std::ofstream out(conf.output_path + "-carriers.txt");
      for (size_t r = 0; r + 1 < row_offsets.size(); ++r) {
        for (int64_t q = row_offsets[r]; q < row_offsets[r + 1]; ++q) out << (q > row_offsets[r] ? " " : "") << sample_idx[(size_t)q];
        out << "\n";
      }
    }
    return 0;
  }
  if (sample_idx.empty()) sample_idx.push_back(0);

  // the layout of S (pcoa_plan_layout; the rule is in pcoa.h): decided before any engine exists.  auto with k > 1 asks every
  // device of --gpu-map for its free memory (engines sharing a device split it) and keeps the full layout where it fits or
  // where the devices cannot be asked (engine creation then reports why)
  std::vector<std::pair<int32_t, int32_t>> strips;   // empty: the full layout
  {
    const int k = conf.gpus;
    int32_t request = conf.layout == "full" ? PCOA_LAYOUT_FULL : conf.layout == "strips" ? PCOA_LAYOUT_STRIPS : PCOA_LAYOUT_AUTO;
    if (request == PCOA_LAYOUT_STRIPS && k > n)
      die("--layout strips: " + std::to_string(k) + " owners for " + std::to_string(n) + " samples; every owner needs a column");
    std::vector<int64_t> free_bytes((size_t)k, 0);
    if (request == PCOA_LAYOUT_AUTO && k > 1 && k <= n) {   // (one engine: full, without asking a device)
      std::map<int, int64_t> dev_free;
      for (int d : conf.gpu_map) {
        int64_t fr = 0;
        if (dev_free.count(d)) continue;
        if (pcoa_device_memory(d, &fr, nullptr) != PCOA_OK) {
          request = PCOA_LAYOUT_FULL;
          break;
        }
        dev_free[d] = fr;
      }
      for (int g = 0; g < k && request == PCOA_LAYOUT_AUTO; ++g)
        free_bytes[(size_t)g] = dev_free[conf.gpu_map[(size_t)g]] /
                                (int64_t)std::count(conf.gpu_map.begin(), conf.gpu_map.end(), conf.gpu_map[(size_t)g]);
    }
    std::vector<int32_t> col0((size_t)k), cols((size_t)k);
    int32_t layout = PCOA_LAYOUT_FULL;
    if (pcoa_plan_layout(n, k, free_bytes.data(), request, &layout, col0.data(), cols.data()) != PCOA_OK)
      die(std::string("pcoa_plan_layout: ") + pcoa_last_error(nullptr));
    if (layout == PCOA_LAYOUT_STRIPS) {
      if (conf.outlier_iterations > 0) die(kStripsRefuseOutliers);   // --layout auto resolved to strips
      if (conf.related) die(kStripsRefuseRelated);
      if (conf.king) die(kStripsRefuseKing);
      if (conf.similarity_measure != "shared") die(strips_refuse_measure(conf.similarity_measure));
      if (g_calls.on) die(kStripsRefuseMissing);
      if (conf.reduce == "rccl") die("the strip layout has no reduction step: it cannot take --reduce rccl");
      for (int g = 0; g < k; ++g) strips.emplace_back(col0[(size_t)g], cols[(size_t)g]);
    }
  }
  const int per_owner = strips.empty() ? 1 : conf.gpus;   // every owner ingests every variant: its counts are k-fold

  // getSimilarityMatrix (:182-191) and computePca (:198-231) on the GPU(s)
  // The RDD[Seq[Int]] rows go over as what they are: carrier lists (pcoa_accumulate_calls_ex).  The device checks the
  // range of every index and finds a list that names a callset twice -- mergeDatasets can produce one when a key occurs
  // twice inside one VCF; the reference's double loop counts such a repeat with multiplicity (:187), and the engine then
  // redoes that chunk on the int8 kernel.  (Until r05 the rows were re-packed into bitsets here by one host thread, ~1 us
  // per variant of a dense cohort: the lists themselves cross the link at 37 M variants/s.)
  StreamStats stream_stats;
  std::atomic<int64_t> fed_as_bits{0}, fed_as_lists{0}, joined_rows{0};
  std::vector<unsigned char*> blocks;  // page-locked blocks of the streaming reader, four per engine (filled by `prepare`)
  ProjectionFeeder* proj_feeder = nullptr;   // --project-input-path: every row to both engines (feed below)
  // engine g takes shard `shard` of `k`: the contiguous range shard_range(shard, k, rows) -- the reference's partitions (:184);
  // under the strip layout every engine takes shard 0 of 1, i.e. every variant
  std::function<void(int, int, int, pcoa_ctx*)> feed = [&](int g, int shard, int k, pcoa_ctx* ctx) {
    if (stream_plink) {
      unsigned char* const four[4] = {blocks[(size_t)(4 * g)], blocks[(size_t)(4 * g + 1)], blocks[(size_t)(4 * g + 2)], blocks[(size_t)(4 * g + 3)]};
      stream_plink_shard(conf, plink, shard, k, ctx, &stream_stats, four);
      return;
    }
    CarrierFeeder feeder;   // one per engine thread
    const unsigned feed_threads = std::max(1u, std::min<unsigned>(conf.ingest_threads > 0 ? (unsigned)conf.ingest_threads : std::thread::hardware_concurrency(), 16u) / (unsigned)conf.gpus);
    struct Tally {   // the engines' totals, for the stderr line
      CarrierFeeder& f; std::atomic<int64_t>& bits; std::atomic<int64_t>& lists;
      ~Tally() { bits += f.rows_as_bits; lists += f.rows_as_lists; }
    } tally{feeder, fed_as_bits, fed_as_lists};
    auto give = [&](const int32_t* idx, const int64_t* offs, int64_t rows) {
      if (proj_feeder) proj_feeder->feed(n, idx, offs, rows, feed_threads);
      else feeder.feed(ctx, conf, n, idx, offs, rows, feed_threads);
    };
    if (stream_join) {   // pass 2: key partitions q = g, g + k, ..: read back, join / merge, feed
      std::vector<int32_t> idx;
      std::vector<int64_t> offs;
      for (int q = shard; q < spill.parts; q += k) {
        std::vector<std::vector<Variant>> sets;
        for (int sset = 0; sset < spill.sets; ++sset) sets.push_back(spill.read(sset, q));
        std::vector<std::vector<int32_t>> rows;
        join_or_merge(sets, rows);
        idx.clear();
        offs.assign(1, 0);
        for (const auto& calls : rows) {
          if (calls.empty()) continue;   // getCallsRdd (:166)
          idx.insert(idx.end(), calls.begin(), calls.end());
          offs.push_back((int64_t)idx.size());
        }
        if (offs.size() > 1) {
          give(idx.data(), offs.data(), (int64_t)offs.size() - 1);
          joined_rows += (int64_t)offs.size() - 1;
        }
      }
      return;
    }
    if (stream_vcf) {
      std::vector<int32_t> idx;
      std::vector<int64_t> offs;
      const std::function<void(std::vector<ParsedLine>&)> sink = [&](std::vector<ParsedLine>& parsed) {
        idx.clear();
        offs.assign(1, 0);
        for (auto& pl : parsed) {
          if (!pl.keep) continue;
          if (conf.has_maf && !(pl.v.has_af && pl.v.af >= conf.min_allele_frequency)) continue;   // filterDataset (:96-108)
          if (pl.v.carriers.empty()) continue;                                                     // getCallsRdd (:166)
          idx.insert(idx.end(), pl.v.carriers.begin(), pl.v.carriers.end());
          offs.push_back((int64_t)idx.size());
          if (g_want_meta) fed_meta.push_back(pl.v.meta);
        }
        if (offs.size() > 1) {
          give(idx.data(), offs.data(), (int64_t)offs.size() - 1);
          streamed_variants += (int64_t)offs.size() - 1;
        }
      };
      (void)load_vcf(conf.input_path[0], stream_stem, stream_regions, 0, false, conf.ingest_threads, &sink);
      return;
    }
    int64_t ra, rb;
    shard_range(shard, k, (int64_t)row_offsets.size() - 1, &ra, &rb);
    if (rb <= ra) return;
    give(sample_idx.data(), row_offsets.data() + ra, rb - ra);
  };
  std::string how;
  double feed_s = 0, warmup_s = 0;
  auto prepare = [&](const std::vector<pcoa_ctx*>& engines) {
    if (g_ld.on) {
      g_ld.meta = stream_plink ? &plink.meta : &fed_meta;
      check(engines[0], pcoa_ld_begin(engines[0], conf.ld_window, conf.ld_r2, PCOA_LD_ACCUMULATE), "pcoa_ld_begin");
    }
    if (g_calls.on) {   // the companion beside engine 0, with its operand buffers
      if (pcoa_create(&g_calls.companion, n, conf.gpu_map[0], PCOA_FLAG_DEFAULT) != PCOA_OK)
        die(std::string("pcoa_create (the call companion): ") + pcoa_last_error(nullptr));
      check(g_calls.companion, pcoa_reserve(g_calls.companion, (int64_t)1 << 20, 0), "pcoa_reserve");
    }
    if (g_king.on)      // the five planes beside engine 0, with their operand buffers
      for (pcoa_ctx*& p : g_king.planes) {
        if (pcoa_create(&p, n, conf.gpu_map[0], PCOA_FLAG_DEFAULT) != PCOA_OK)
          die(std::string("pcoa_create (a plane of --king-cutoff): ") + pcoa_last_error(nullptr));
        check(p, pcoa_reserve(p, (int64_t)1 << 20, 0), "pcoa_reserve");
      }
    if (!stream_plink) return;
    for (int q = 0; q < 4 * conf.gpus; ++q) {
      void* b = nullptr;
      if (pcoa_host_alloc_pinned((size_t)conf.stream_rows * plink.bpv, &b) != PCOA_OK) die("pcoa_host_alloc_pinned failed");
      blocks.push_back(static_cast<unsigned char*>(b));
    }
    if (conf.plink_decode == "host") return;
    // the rest of an executor's warm-up (pcoa_reserve covers the operand buffers): one block of homozygous-reference rows
    // through the device decode -- staging slots, the bitset tile and the kernels' code objects exist before the first real
    // block; it adds nothing to S and is taken out of the books again
    const bool ref_a1 = conf.plink_ref_allele == "a1";
    const double tw0 = now_s();
    for (int g = 0; g < conf.gpus; ++g) {
      unsigned char* b = blocks[(size_t)(4 * g)];
      int64_t r0 = 0, r1 = 0;
      shard_range(strips.empty() ? g : 0, strips.empty() ? conf.gpus : 1, (int64_t)plink.keep.size(), &r0, &r1);
      const int64_t wrows = std::max<int64_t>(1, std::min<int64_t>(conf.stream_rows, r1 - r0));   // never more than the shard itself
      std::memset(b, ref_a1 ? 0x00 : 0xFF, (size_t)wrows * plink.bpv);
      pcoa_ctx* e = engines[(size_t)g];
      check(e, pcoa_accumulate_plink_bed(e, b, wrows, (int64_t)plink.bpv, ref_a1 ? 1 : 0, 0), "warm-up");
      check(e, pcoa_sync(e), "warm-up");
      check(e, pcoa_reset(e), "warm-up");
      check(e, pcoa_reset_timings(e), "warm-up");
    }
    warmup_s = now_s() - tw0;
  };
  if (projecting) {
    // PCA of the reference cohort on a full engine over N_ref, the other samples placed onto it (pcoa_project) from a strip owner
    // over columns [N_ref, N): the cross block S[0:N_ref, N_ref:N] (and the rows below it, unused)
    const int32_t n_new = n - n_ref;
    if (n_ref <= 0 || n_new <= 0) die("--project-input-path: both the reference and the projected inputs need samples");
    if (conf.num_pc < 2) die("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2");
    pcoa_ctx* ref = nullptr;
    pcoa_ctx* cross = nullptr;
    if (pcoa_create(&ref, n_ref, conf.gpu, PCOA_FLAG_DEFAULT) != PCOA_OK) die(std::string("pcoa_create: ") + pcoa_last_error(nullptr));
    if (pcoa_create_strip(&cross, n, n_ref, n_new, conf.gpu, PCOA_FLAG_DEFAULT) != PCOA_OK)
      die(std::string("pcoa_create_strip: ") + pcoa_last_error(nullptr));
    check(ref, pcoa_reserve(ref, (int64_t)1 << 20, conf.num_pc), "pcoa_reserve");
    check(cross, pcoa_reserve(cross, (int64_t)1 << 20, 0), "pcoa_reserve");
    ProjectionFeeder pf;
    pf.ref = ref;
    pf.cross = cross;
    proj_feeder = &pf;
    const double t0 = now_s();
    feed(0, 0, 1, ref);
    check(ref, pcoa_gram_finalize(ref), "getSimilarityMatrix");
    check(cross, pcoa_gram_finalize(cross), "getSimilarityMatrix");
    feed_s = now_s() - t0;
    if (stream_join) spill.remove_all();
    std::fprintf(stderr, "getSimilarityMatrix: %lld variants in %.3f s (reference engine over %d samples, strip owner over columns "
                 "[%d, %d) of %d; every row packed once as a carrier bitset for both)\n", (long long)pf.rows_fed, feed_s, n_ref, n_ref, n, n);
    if (!conf.dump_similarity.empty()) {   // the reference's S (N_ref x N_ref)
      std::vector<int64_t> sim((size_t)n_ref * (size_t)n_ref);
      check(ref, pcoa_gram_read_i64(ref, sim.data()), "dump-similarity");
      std::ofstream out(conf.dump_similarity, std::ios::binary);
      out.write(reinterpret_cast<const char*>(sim.data()), (std::streamsize)(sim.size() * sizeof(int64_t)));
      if (!out) die("cannot write " + conf.dump_similarity);
    }
    std::vector<double> comps((size_t)conf.num_pc * (size_t)n_ref), lam((size_t)conf.num_pc), coords((size_t)conf.num_pc * (size_t)n_new);
    int32_t nonzero = 0;
    check(ref, pcoa_compute(ref, conf.num_pc, comps.data(), lam.data(), &nonzero), "computePca");
    std::printf("Non zero rows in matrix: %d / %d.\n", nonzero, n_ref);
    check(ref, pcoa_project(ref, cross, conf.num_pc, comps.data(), lam.data(), coords.data()), "project");
    std::printf("Projected %d samples onto %d principal components of %d reference samples.\n", n_new, conf.num_pc, n_ref);
    std::vector<OutRow> rows;
    for (int32_t i = 0; i < n; ++i) {
      const bool r = i < n_ref;
      const size_t at = r ? (size_t)i : (size_t)(i - n_ref), ld = r ? (size_t)n_ref : (size_t)n_new;
      const std::vector<double>& v = r ? comps : coords;
      rows.push_back({names[(size_t)i], ids[(size_t)i].substr(0, ids[(size_t)i].find('-')), v[at], v[at + ld]});
    }
    emit_result(conf, rows);
    pcoa_timings t;
    if (pcoa_get_timings(ref, &t) == PCOA_OK)
      std::fprintf(stderr, "Variants accumulated: %lld; Gram kernel %.3f ms; PCoA %.3f ms\n", (long long)t.gram_variants,
                   1e3 * t.gram_kernel_seconds, 1e3 * t.compute_total_seconds);
    pcoa_destroy(cross);
    pcoa_destroy(ref);
    return 0;
  }
  std::vector<pcoa_ctx*> owners = run_engines(conf, n, strips, feed, &how, &feed_s, prepare);
  pcoa_ctx* ctx = owners[0];   // (--outlier-iterations replaces it by its subsets)
  if (stream_join) {
    std::fprintf(stderr, "%zu variant set(s) through %d key partitions: %lld records, %.1f MB of spill files in %s\n",
                 conf.input_path.size(), spill.parts, (long long)spilled_records, spill.bytes / 1e6, spill.dir.c_str());
    spill.remove_all();
  }
  if (stream_plink) fed_meta = plink.meta;                 // one engine: every kept line, in file order
  if (stream_join || data.size() > 1) fed_meta_known = false;
  for (pcoa_ctx* o : owners) check(o, pcoa_gram_finalize(o), "getSimilarityMatrix");
  // --grm: what the engine will decompose (again after every subset, for the reduced cohort)
  auto grm_report = [&](pcoa_ctx* eng) {
    int64_t variants = 0, used = 0, store = 0;
    if (pcoa_grm_info(eng, &variants, &used, &store) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(eng));
    std::fprintf(stderr, "Standardised genotypes: %lld of %lld variants used (min MAF %g), store %lld bytes\n", (long long)used,
                 (long long)variants, conf.grm_min_maf, (long long)store);
  };
  // --grm-ld-window: the resident store is pruned, a break in front of the first variant of every new contig (with
  // --grm-keep-samples / --grm-remove-samples / --grm-outlier-iterations: every round's engine, whose frequencies name the candidates)
  auto grm_ld_prune_now = [&](pcoa_ctx* eng) {
    int64_t variants = 0;
    if (pcoa_grm_info(eng, &variants, nullptr, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(eng));
    {
      const bool known = fed_meta_known && (int64_t)fed_meta.size() == variants;
      std::vector<int64_t> breaks;
      if (known)
        for (int64_t v = 1; v < variants; ++v)
          if (fed_meta[(size_t)v].contig != fed_meta[(size_t)v - 1].contig) breaks.push_back(v);
      int64_t cand = 0, kept = 0;
      check(eng, pcoa_grm_ld_prune(eng, conf.grm_ld_window, conf.grm_ld_r2, breaks.empty() ? nullptr : breaks.data(), (int64_t)breaks.size(),
                                   &cand, &kept), "pcoa_grm_ld_prune");
      std::printf("GRM LD pruning: kept %lld of %lld candidate variants (%lld in the store), window %d, r2 %g\n", (long long)kept,
                  (long long)cand, (long long)variants, conf.grm_ld_window, conf.grm_ld_r2);
      pcoa_grm_ld_stats gs;
      check(eng, pcoa_get_grm_ld_stats(eng, &gs, sizeof(gs)), "pcoa_get_grm_ld_stats");
      std::fprintf(stderr, "GRM LD pruning: %lld pairs; band %.3f ms, resolve %.3f ms, scan %.3f ms\n", (long long)gs.grm_ld_pairs,
                   1e3 * gs.grm_ld_band_seconds, 1e3 * gs.grm_ld_resolve_seconds, 1e3 * gs.grm_ld_scan_seconds);
      if (!conf.grm_ld_output_path.empty()) {
        std::vector<uint8_t> keep((size_t)std::max<int64_t>(variants, 1));
        check(eng, pcoa_grm_ld_mask(eng, 0, variants, keep.data()), "pcoa_grm_ld_mask");
        std::ofstream out(conf.grm_ld_output_path);
        for (int64_t v = 0; v < variants; ++v) {
          if (known) out << v << "\t" << fed_meta[(size_t)v].contig << "\t" << fed_meta[(size_t)v].pos << "\t" << fed_meta[(size_t)v].id;
          else out << v << "\t.\t.\t.";
          out << "\t" << (keep[(size_t)v] ? 1 : 0) << "\n";
        }
        if (!out) die("cannot write " + conf.grm_ld_output_path);
      }
    }
  };
  if (conf.grm) {
    check(ctx, pcoa_grm_set_min_maf(ctx, conf.grm_min_maf), "pcoa_grm_set_min_maf");
    check(ctx, pcoa_grm_set_variant_filters(ctx, conf.grm_geno, conf.grm_hwe), "pcoa_grm_set_variant_filters");   // every subset inherits them
    grm_report(ctx);
    if (conf.has_grm_geno || conf.has_grm_hwe || conf.has_grm_mind || !conf.grm_variant_qc_output_path.empty() ||
        !conf.grm_sample_qc_output_path.empty()) {
      // --grm-mind and the two QC files, on the engine of the whole fileset straight after the feed: the variant file (counts,
      // missing share, HWE p and used_v of the fed cohort, in the fp64 expressions of pcoa.h), the sample file (before anyone
      // is removed), the stderr line
      int64_t total = 0;
      if (pcoa_grm_info(ctx, &total, nullptr, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(ctx));
      if (!conf.grm_variant_qc_output_path.empty()) {
        std::vector<int32_t> cnt((size_t)std::max<int64_t>(total, 1) * 3);
        std::vector<double> p((size_t)std::max<int64_t>(total, 1));
        check(ctx, pcoa_grm_counts(ctx, 0, total, cnt.data()), "pcoa_grm_counts");
        check(ctx, pcoa_grm_hwe(ctx, 0, total, p.data()), "pcoa_grm_hwe");
        const bool known = fed_meta_known && (int64_t)fed_meta.size() == total;
        FILE* f = std::fopen(conf.grm_variant_qc_output_path.c_str(), "w");
        if (!f) die("cannot write " + conf.grm_variant_qc_output_path);
        for (int64_t v = 0; v < total; ++v) {
          const int32_t nv = cnt[(size_t)v * 3], h = cnt[(size_t)v * 3 + 1], o = cnt[(size_t)v * 3 + 2];
          const int64_t a = (int64_t)h + 2 * (int64_t)o;
          bool used = nv > 0 && a > 0 && a < 2 * (int64_t)nv &&
                      (double)std::min<int64_t>(a, 2 * (int64_t)nv - a) >= conf.grm_min_maf * (2.0 * (double)nv);
          used = used && (double)(n - nv) <= conf.grm_geno * (double)n;
          if (conf.grm_hwe != 0.0) used = used && p[(size_t)v] >= conf.grm_hwe;
          if (known)
            std::fprintf(f, "%lld\t%s\t%s\t%s", (long long)v, fed_meta[(size_t)v].contig.c_str(),
                         std::to_string(fed_meta[(size_t)v].pos).c_str(), fed_meta[(size_t)v].id.c_str());
          else
            std::fprintf(f, "%lld\t.\t.\t.", (long long)v);
          std::fprintf(f, "\t%d\t%d\t%d\t%.6f\t%.17g\t%d\n", nv, h, o, (double)(n - nv) / (double)n, p[(size_t)v], used ? 1 : 0);
        }
        if (std::fclose(f) != 0) die("cannot write " + conf.grm_variant_qc_output_path);
      }
      int32_t mind_gone = 0;
      if (conf.has_grm_mind || !conf.grm_sample_qc_output_path.empty()) {
        std::vector<int64_t> sc((size_t)n * 3);
        check(ctx, pcoa_grm_sample_counts(ctx, PCOA_GRM_ROWS_ALL, sc.data()), "pcoa_grm_sample_counts");
        std::vector<char> stay((size_t)n, 1);
        if (conf.has_grm_mind && total > 0)
          for (int32_t i = 0; i < n; ++i)
            stay[(size_t)i] = (double)(total - sc[(size_t)i * 3]) / (double)total > conf.grm_mind ? 0 : 1;
        if (!conf.grm_sample_qc_output_path.empty()) {
          FILE* f = std::fopen(conf.grm_sample_qc_output_path.c_str(), "w");
          if (!f) die("cannot write " + conf.grm_sample_qc_output_path);
          for (int32_t i = 0; i < n; ++i) {
            const int64_t called = sc[(size_t)i * 3];
            std::fprintf(f, "%s\t%lld\t%lld\t%lld\t%.6f\t%.6f\t%d\n", names[(size_t)i].c_str(), (long long)called,
                         (long long)sc[(size_t)i * 3 + 1], (long long)sc[(size_t)i * 3 + 2],
                         total ? (double)called / (double)total : 0.0, called ? (double)sc[(size_t)i * 3 + 1] / (double)called : 0.0,
                         stay[(size_t)i] ? 1 : 0);
          }
          if (std::fclose(f) != 0) die("cannot write " + conf.grm_sample_qc_output_path);
        }
        if (conf.has_grm_mind) {
          for (int32_t i = 0; i < n; ++i)
            if (!stay[(size_t)i]) {
              ++mind_gone;
              grm_mind_gone.push_back(i);
            }
          if (mind_gone > 0) {   // the samples --grm-mind keeps join (or become) the list
            std::vector<int32_t> both;
            if (grm_has_list) {
              for (int32_t i : grm_listed)
                if (stay[(size_t)i]) both.push_back(i);
            } else {
              for (int32_t i = 0; i < n; ++i)
                if (stay[(size_t)i]) both.push_back(i);
            }
            const int32_t least = std::max(32, conf.num_pc + 1);
            if ((int32_t)both.size() < least)
              die("--grm --grm-mind leaves " + std::to_string(both.size()) + " of " + std::to_string(n) + " samples, fewer than the " +
                  std::to_string(least) + " a GRM engine with " + std::to_string(conf.num_pc) + " principal components needs");
            grm_listed.swap(both);
            grm_has_list = true;
          }
        }
      }
      pcoa_grm_qc_stats qs;
      check(ctx, pcoa_get_grm_qc_stats(ctx, &qs, sizeof(qs)), "pcoa_get_grm_qc_stats");
      std::fprintf(stderr, "GRM QC: removed %lld variant(s) by MAF, %lld by missing rate, %lld by HWE; %d sample(s) by call rate\n",
                   (long long)qs.grm_qc_fail_maf, (long long)qs.grm_qc_fail_missing, (long long)qs.grm_qc_fail_hwe, mind_gone);
    }
    if (conf.grm_ld_window > 0 && !grm_rounds) grm_ld_prune_now(ctx);
  }
  if (g_ld.on) {
    pcoa_ld_stats ls;
    check(ctx, pcoa_get_ld_stats(ctx, &ls, sizeof(ls)), "pcoa_get_ld_stats");
    check(ctx, pcoa_ld_end(ctx), "pcoa_ld_end");
    std::printf("LD pruning: kept %lld of %lld variants (%lld monomorphic)\n", (long long)ls.ld_kept, (long long)ls.ld_variants,
                (long long)ls.ld_monomorphic);
    std::fprintf(stderr, "LD pruning: window %d, r2 %s; %lld pairs; count %.3f ms, band %.3f ms, resolve %.3f ms, compaction %.3f ms\n",
                 conf.ld_window, java_double(conf.ld_r2).c_str(), (long long)ls.ld_pairs, 1e3 * ls.ld_count_seconds, 1e3 * ls.ld_band_seconds,
                 1e3 * ls.ld_resolve_seconds, 1e3 * ls.ld_compact_seconds);
    if (!conf.ld_output_path.empty()) {
      const bool known = fed_meta_known && (int64_t)fed_meta.size() == g_ld.fed;
      std::ofstream out(conf.ld_output_path);
      for (int64_t v = 0; v < g_ld.fed; ++v) {
        if (known) out << v << "\t" << fed_meta[(size_t)v].contig << "\t" << fed_meta[(size_t)v].pos << "\t" << fed_meta[(size_t)v].id;
        else out << v << "\t.\t.\t.";
        out << "\t" << (g_ld.keep[(size_t)v] ? 1 : 0) << "\n";
      }
      if (!out) die("cannot write " + conf.ld_output_path);
    }
  }
  {
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    if (stream_plink)
      std::fprintf(stderr, "Streamed %lld variants x %d samples from %s.bed in %.3f s = %.1f M variants/s (ingest -> reduced S; engines "
                   "already created and a warm-up block of %.3f s per run -- first-use allocation, code-object load -- NOT included; %s; "
                   "slowest shard: reads %.3f s, feed calls %.3f s; %s decode); peak RSS %.0f MB\n", (long long)stream_stats.variants / per_owner, n,
                   plink.prefix.c_str(), feed_s, stream_stats.variants / per_owner / feed_s / 1e6, warmup_s, how.c_str(), stream_stats.read_s,
                   stream_stats.feed_s, conf.plink_decode.c_str(), ru.ru_maxrss / 1024.0);
    else
      std::fprintf(stderr, "getSimilarityMatrix: %zu variants in %.3f s (%s%s; %lld rows as carrier bitsets, %lld as carrier lists); peak RSS %.0f MB\n",
                   stream_join ? (size_t)(joined_rows.load() / per_owner) : stream_vcf ? (size_t)(streamed_variants / per_owner) : row_offsets.size() - 1,
                   feed_s, how.c_str(),
                   stream_join ? "; sets streamed into key-partitioned spill files, joined one partition at a time" :
                   stream_vcf ? "; the VCF streamed block by block: read + parse + feed" : "", (long long)(fed_as_bits.load() / per_owner),
                   (long long)(fed_as_lists.load() / per_owner), ru.ru_maxrss / 1024.0);
  }
  if (!conf.dump_similarity.empty()) {  // all N^2 entries, as matrix.iterator emits them (:189)
    std::vector<int64_t> sim((size_t)n * (size_t)n);
    if (strips.empty()) {
      check(ctx, pcoa_gram_read_i64(ctx, sim.data()), "dump-similarity");
    } else {   // each owner's [N][cols] into its columns
      std::vector<int64_t> part;
      for (size_t g = 0; g < owners.size(); ++g) {
        const int32_t c0 = strips[g].first, w = strips[g].second;
        part.resize((size_t)n * (size_t)w);
        check(owners[g], pcoa_gram_read_i64(owners[g], part.data()), "dump-similarity");
        for (int32_t r = 0; r < n; ++r)
          std::copy(part.begin() + (size_t)r * w, part.begin() + (size_t)(r + 1) * w, sim.begin() + (size_t)r * n + c0);
      }
    }
    std::ofstream out(conf.dump_similarity, std::ios::binary);
    out.write(reinterpret_cast<const char*>(sim.data()), (std::streamsize)(sim.size() * sizeof(int64_t)));
    if (!out) die("cannot write " + conf.dump_similarity);
  }
  if (conf.num_pc < 2)  // the reference reads array(i + pca.numRows) unconditionally (:230)
    die("computePca emits exactly PC1 and PC2 (VariantsPca.scala:229-230); --num-pc must be >= 2");
  std::vector<double> comps((size_t)conf.num_pc * (size_t)n), lam((size_t)conf.num_pc);
  int32_t nonzero = 0;
  double gram_s_before = 0.0;             // Gram kernel seconds of engines that --outlier-iterations has replaced
  std::vector<int32_t> kept((size_t)n);   // original index of every sample of the current cohort
  for (int32_t i = 0; i < n; ++i) kept[(size_t)i] = i;
  if (conf.similarity_measure != "shared")   // on the engine that runs computePca (engine 0 after a reduction); its subsets inherit it
    check(ctx, pcoa_set_similarity(ctx, conf.similarity_kind()), "set-similarity");
  if (g_calls.on) {
    // --missing-calls pairwise: bound just before the screen and the rounds, V = the variants fed; the subsets get companions
    // of their own (pcoa_create_subset).  diag(Q) = the missing calls of every sample, by the screen's count-only call
    pcoa_ctx* q = g_calls.companion;
    check(q, pcoa_gram_finalize(q), "getSimilarityMatrix");
    const int64_t fed = (int64_t)std::count(plink.keep.begin(), plink.keep.end(), (char)1);
    std::vector<int64_t> miss((size_t)n);
    int64_t none = 0, total_missing = 0;
    check(q, pcoa_similar_pairs(q, 1.0, nullptr, 0, &none, miss.data()), "pcoa_similar_pairs");
    for (int64_t m : miss) total_missing += m;
    check(ctx, pcoa_set_call_companion(ctx, q, fed), "pcoa_set_call_companion");
    std::printf("Missing calls: %lld of %lld genotypes (pairwise-complete similarity)\n", (long long)total_missing, (long long)(fed * n));
    if (!conf.call_rate_output_path.empty()) {
      std::ofstream out(conf.call_rate_output_path);
      char buf[64];
      for (int32_t i = 0; i < n; ++i) {
        const int64_t c = fed - miss[(size_t)i];
        std::snprintf(buf, sizeof(buf), "%.6f", fed ? (double)c / (double)fed : 0.0);
        out << names[(size_t)i] << "\t" << c << "\t" << fed << "\t" << buf << "\n";
      }
      if (!out) die("cannot write " + conf.call_rate_output_path);
    }
  }
  // --remove-related / --king-remove: the engine replaced by its subset over the samples a screen keeps (one gather of S, no
  // variant read twice); `gone` is sorted
  auto drop_samples = [&](const std::vector<int32_t>& gone, const char* remove_flag, const char* threshold_flag) {
    if (gone.empty()) return;
    const int32_t least = std::max(3, conf.num_pc + 1);
    if (n - (int32_t)gone.size() < least)
      die(std::string(remove_flag) + " would leave " + std::to_string(n - (int32_t)gone.size()) + " of " + std::to_string(n) +
          " samples, fewer than the " + std::to_string(least) + " that " + std::to_string(conf.num_pc) +
          " principal components need; raise " + threshold_flag);
    std::vector<int32_t> keep;
    size_t g = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (g < gone.size() && gone[g] == i) ++g;
      else keep.push_back(i);
    }
    pcoa_ctx* sub = nullptr;
    check(ctx, pcoa_create_subset(&sub, ctx, keep.data(), (int32_t)keep.size()), "pcoa_create_subset");
    pcoa_timings tp;   // the Gram kernels ran on the predecessor: its time goes into the closing line
    if (pcoa_get_timings(ctx, &tp) == PCOA_OK) gram_s_before += tp.gram_kernel_seconds;
    pcoa_destroy(ctx);
    ctx = owners[0] = sub;
    kept.swap(keep);
  };
  if (conf.related) {
    // --related-min-jaccard X, before the first computePca: the screen of S on the device.  The rule, as pcoa.h and
    // variants_pca.py's related_pairs_rule state it: with d_i = S(i, i) and U = d_i + d_j - S(i, j), the pair (i, j), i < j, is
    // reported iff U > 0 and (double)S(i, j) >= X * (double)U.  Then the pair file, one stderr line, and with --remove-related
    // the engine replaced by its subset over the kept samples (one gather of S, no variant read twice)
    std::vector<pcoa_pair> pairs((size_t)std::min<int64_t>(conf.related_max_pairs, (int64_t)n * (n - 1) / 2));
    std::vector<int64_t> diag((size_t)n);
    int64_t n_found = 0;
    check(ctx, pcoa_similar_pairs(ctx, conf.related_min_jaccard, pairs.empty() ? nullptr : pairs.data(), (int64_t)pairs.size(), &n_found,
                                  diag.data()), "pcoa_similar_pairs");
    if (n_found > conf.related_max_pairs)
      die("--related-min-jaccard " + java_double(conf.related_min_jaccard) + " reports " + std::to_string(n_found) +
          " pairs, more than --related-max-pairs " + std::to_string(conf.related_max_pairs) + " takes; raise --related-max-pairs or the threshold");
    pairs.resize((size_t)n_found);
    if (!conf.related_output_path.empty()) {
      std::ofstream out(conf.related_output_path);
      out << "name_i\tname_j\tshared\td_i\td_j\tjaccard\n";
      for (const pcoa_pair& p : pairs) {
        const int64_t di = diag[(size_t)p.i], dj = diag[(size_t)p.j], u = di + dj - p.shared;
        out << names[(size_t)p.i] << "\t" << names[(size_t)p.j] << "\t" << p.shared << "\t" << di << "\t" << dj << "\t"
            << java_double((double)p.shared / (double)u) << "\n";
      }
      if (!out) die("cannot write " + conf.related_output_path);
    }
    const std::vector<int32_t> gone = conf.remove_related ? related_removal(pairs, n) : std::vector<int32_t>();
    std::string gone_names;
    for (int32_t i : gone) gone_names += (gone_names.empty() ? ": " : ", ") + names[(size_t)i];
    std::fprintf(stderr, "Related pairs: %lld at jaccard >= %s; removed %zu sample(s)%s\n", (long long)n_found,
                 java_double(conf.related_min_jaccard).c_str(), gone.size(), gone_names.c_str());
    drop_samples(gone, "--remove-related", "--related-min-jaccard");
  }
  if (conf.king) {
    // --king-cutoff X, before the first computePca: the KING-robust screen over the five planes.  The rule, as pcoa.h and
    // variants_pca.py's king_pairs_rule state it: the pair (i, j), i < j, is reported iff het_sum > 0 and
    // (double)(hethet - 2 ibs0) >= X * (double)het_sum.  The planes are destroyed right after the screen; then the pair file,
    // one stderr line, and with --king-remove the removal rule and the subset of --remove-related
    std::vector<pcoa_king_pair> found((size_t)std::min<int64_t>(conf.king_max_pairs, (int64_t)n * (n - 1) / 2));
    int64_t n_found = 0;
    check(g_king.planes[0], pcoa_king_pairs(g_king.planes, conf.king_cutoff, found.empty() ? nullptr : found.data(), (int64_t)found.size(),
                                            &n_found, nullptr, nullptr), "pcoa_king_pairs");
    for (pcoa_ctx*& p : g_king.planes) {
      pcoa_destroy(p);
      p = nullptr;
    }
    if (n_found > conf.king_max_pairs)
      die("--king-cutoff " + java_double(conf.king_cutoff) + " reports " + std::to_string(n_found) + " pairs, more than --king-max-pairs " +
          std::to_string(conf.king_max_pairs) + " takes; raise --king-max-pairs or the cutoff");
    found.resize((size_t)n_found);
    if (!conf.king_output_path.empty()) {
      std::ofstream out(conf.king_output_path);
      out << "name_i\tname_j\thethet\tibs0\thet_sum\tkinship\n";
      for (const pcoa_king_pair& p : found)
        out << names[(size_t)p.i] << "\t" << names[(size_t)p.j] << "\t" << p.hethet << "\t" << p.ibs0 << "\t" << p.het_sum << "\t"
            << java_double((double)(p.hethet - 2 * p.ibs0) / (double)p.het_sum) << "\n";
      if (!out) die("cannot write " + conf.king_output_path);
    }
    std::vector<pcoa_pair> pairs(found.size());
    for (size_t k = 0; k < found.size(); ++k) pairs[k] = pcoa_pair{found[k].i, found[k].j, 0};
    const std::vector<int32_t> gone = conf.king_remove ? related_removal(pairs, n) : std::vector<int32_t>();
    std::string gone_names;
    for (int32_t i : gone) gone_names += (gone_names.empty() ? ": " : ", ") + names[(size_t)i];
    std::fprintf(stderr, "KING pairs: %lld at kinship >= %s; removed %zu sample(s)%s\n", (long long)n_found,
                 java_double(conf.king_cutoff).c_str(), gone.size(), gone_names.c_str());
    drop_samples(gone, "--king-remove", "--king-cutoff");
  }
  pcoa_ctx* const grm_full = conf.grm ? ctx : nullptr;   // the engine of the whole fileset (--grm-project-removed subsets it once more)
  // pcoa_create_grm_subset of src (n_src samples) over keep, and the stderr lines: what was gathered and, for a panel, what the
  // reduced cohort's engine will decompose
  auto grm_subset = [&](pcoa_ctx* src, int32_t n_src, const std::vector<int32_t>& keep, int32_t kind) {
    pcoa_grm_subset_stats s0, s1;
    check(src, pcoa_get_grm_subset_stats(src, &s0, sizeof(s0)), "pcoa_get_grm_subset_stats");
    pcoa_ctx* sub = nullptr;
    check(src, pcoa_create_grm_subset(&sub, src, keep.data(), (int32_t)keep.size(), kind), "pcoa_create_grm_subset");
    check(src, pcoa_get_grm_subset_stats(src, &s1, sizeof(s1)), "pcoa_get_grm_subset_stats");
    std::fprintf(stderr, "GRM subset: kept %zu of %d samples, %lld bytes gathered\n", keep.size(), n_src,
                 (long long)(s1.grm_subset_bytes - s0.grm_subset_bytes));
    if (kind == PCOA_GRM_SUBSET_PANEL) grm_report(sub);
    return sub;
  };
  // the cohort's engine is replaced; the whole fileset's stays while --grm-project-removed needs it
  auto grm_replace = [&](pcoa_ctx* sub) {
    if (ctx != grm_full || !conf.grm_project_removed) pcoa_destroy(ctx);
    ctx = owners[0] = sub;
  };
  if (grm_rounds) {
    // --grm-keep-samples / --grm-remove-samples, then the loop of --outlier-iterations below with pcoa_create_grm_subset in
    // pcoa_create_subset's place and the smallest cohort a GRM engine takes
    if (grm_has_list) {
      grm_replace(grm_subset(ctx, n, grm_listed, PCOA_GRM_SUBSET_PANEL));
      kept = grm_listed;
    }
    bool pruned = false;   // ctx carries the prune of --grm-ld-window already
    if (conf.grm_cutoff_given) {
      // --grm-cutoff X: the screen sees the K that would be decomposed: behind the list's subset and one prune of that engine.
      // The rule, as pcoa.h and variants_pca.py's grm_pairs_rule state it: the pair (i, j), i < j, is reported iff K(i, j) >= X.
      // Then the pair file, one stderr line, and with --grm-cutoff-remove the removal rule of --remove-related and the subset
      if (conf.grm_ld_window > 0) {
        grm_ld_prune_now(ctx);
        pruned = true;
      }
      const int32_t m = (int32_t)kept.size();
      const int32_t divisor = conf.grm_cutoff_divisor == "pairwise" ? PCOA_GRM_DIVISOR_PAIRWISE : PCOA_GRM_DIVISOR_USED;
      std::vector<pcoa_grm_pair> found((size_t)std::min<int64_t>(1048576, (int64_t)m * (m - 1) / 2));
      int64_t n_found = 0;
      check(ctx, pcoa_grm_pairs(ctx, conf.grm_cutoff, divisor, 0, found.empty() ? nullptr : found.data(), (int64_t)found.size(), &n_found,
                                nullptr), "pcoa_grm_pairs");
      if (n_found > (int64_t)found.size()) {   // more than the first call's room: the count is known now
        found.resize((size_t)n_found);
        check(ctx, pcoa_grm_pairs(ctx, conf.grm_cutoff, divisor, 0, found.data(), (int64_t)found.size(), &n_found, nullptr), "pcoa_grm_pairs");
      }
      found.resize((size_t)n_found);
      if (conf.has_grm_related_output_path) {
        std::ofstream out(conf.grm_related_output_path);
        out << "name_i\tname_j\tk\tn\n";
        for (const pcoa_grm_pair& p : found)
          out << names[(size_t)kept[(size_t)p.i]] << "\t" << names[(size_t)kept[(size_t)p.j]] << "\t" << java_double(p.k) << "\t" << p.n << "\n";
        if (!out) die("cannot write " + conf.grm_related_output_path);
      }
      std::vector<pcoa_pair> pairs(found.size());
      for (size_t k = 0; k < found.size(); ++k) pairs[k] = pcoa_pair{found[k].i, found[k].j, 0};
      const std::vector<int32_t> gone = conf.grm_cutoff_remove ? related_removal(pairs, m) : std::vector<int32_t>();
      std::fprintf(stderr, "GRM relatedness: %lld pair(s) with K >= %s (divisor %s), removed %zu sample(s)\n", (long long)n_found,
                   java_double(conf.grm_cutoff).c_str(), divisor == PCOA_GRM_DIVISOR_PAIRWISE ? "pairwise" : "used", gone.size());
      if (!gone.empty()) {
        const int32_t least = std::max(32, conf.num_pc + 1);
        if (m - (int32_t)gone.size() < least)
          die("--grm --grm-cutoff-remove leaves " + std::to_string(m - (int32_t)gone.size()) + " of " + std::to_string(m) +
              " samples, fewer than the " + std::to_string(least) + " a GRM engine with " + std::to_string(conf.num_pc) +
              " principal components needs");
        std::vector<int32_t> stay, kept_next;
        size_t g = 0;
        for (int32_t a = 0; a < m; ++a) {
          if (g < gone.size() && gone[g] == a) {
            ++g;
          } else {
            stay.push_back(a);
            kept_next.push_back(kept[(size_t)a]);
          }
        }
        grm_replace(grm_subset(ctx, m, stay, PCOA_GRM_SUBSET_PANEL));
        kept.swap(kept_next);
        pruned = false;
      }
    }
    if (conf.grm_king) {
      // --grm-king-cutoff X: where --grm-cutoff runs, on the variants that would be decomposed (rows used) or on all of them.  The
      // rule, as pcoa.h and variants_pca.py's grm_king_pairs_rule state it: the pair (i, j), i < j, is reported iff het_sum > 0
      // and (double)(hethet - 2 ibs0) >= X * (double)het_sum.  Then the pair file in the format of --king-output-path, one stderr
      // line, and with --grm-king-remove the removal rule of --remove-related and the subset
      if (conf.grm_ld_window > 0 && !pruned) {
        grm_ld_prune_now(ctx);
        pruned = true;
      }
      const int32_t m = (int32_t)kept.size();
      const bool all_rows = conf.grm_king_rows == "all";
      std::vector<pcoa_king_pair> found((size_t)std::min<int64_t>(conf.grm_king_max_pairs, (int64_t)m * (m - 1) / 2));
      int64_t n_found = 0, n_rows = 0;
      check(ctx, pcoa_grm_king_pairs(ctx, all_rows ? PCOA_GRM_ROWS_ALL : PCOA_GRM_ROWS_USED, conf.grm_king_cutoff, 0,
                                     found.empty() ? nullptr : found.data(), (int64_t)found.size(), &n_found, &n_rows, nullptr),
            "pcoa_grm_king_pairs");
      if (n_found > conf.grm_king_max_pairs)
        die("--grm-king-cutoff " + java_double(conf.grm_king_cutoff) + " reports " + std::to_string(n_found) +
            " pairs, more than --grm-king-max-pairs " + std::to_string(conf.grm_king_max_pairs) +
            " takes; raise --grm-king-max-pairs or the cutoff");
      found.resize((size_t)n_found);
      if (conf.has_grm_king_output_path) {
        std::ofstream out(conf.grm_king_output_path);
        out << "name_i\tname_j\thethet\tibs0\thet_sum\tkinship\n";
        for (const pcoa_king_pair& p : found)
          out << names[(size_t)kept[(size_t)p.i]] << "\t" << names[(size_t)kept[(size_t)p.j]] << "\t" << p.hethet << "\t" << p.ibs0 << "\t"
              << p.het_sum << "\t" << java_double((double)(p.hethet - 2 * p.ibs0) / (double)p.het_sum) << "\n";
        if (!out) die("cannot write " + conf.grm_king_output_path);
      }
      std::vector<pcoa_pair> pairs(found.size());
      for (size_t k = 0; k < found.size(); ++k) pairs[k] = pcoa_pair{found[k].i, found[k].j, 0};
      const std::vector<int32_t> gone = conf.grm_king_remove ? related_removal(pairs, m) : std::vector<int32_t>();
      std::fprintf(stderr, "GRM KING: %lld pair(s) with kinship >= %s over %lld row(s) (rows %s), removed %zu sample(s)\n",
                   (long long)n_found, java_double(conf.grm_king_cutoff).c_str(), (long long)n_rows, all_rows ? "all" : "used", gone.size());
      if (!gone.empty()) {
        const int32_t least = std::max(32, conf.num_pc + 1);
        if (m - (int32_t)gone.size() < least)
          die("--grm --grm-king-remove leaves " + std::to_string(m - (int32_t)gone.size()) + " of " + std::to_string(m) +
              " samples, fewer than the " + std::to_string(least) + " a GRM engine with " + std::to_string(conf.num_pc) +
              " principal components needs");
        std::vector<int32_t> stay, kept_next;
        size_t g = 0;
        for (int32_t a = 0; a < m; ++a) {
          if (g < gone.size() && gone[g] == a) {
            ++g;
          } else {
            stay.push_back(a);
            kept_next.push_back(kept[(size_t)a]);
          }
        }
        grm_replace(grm_subset(ctx, m, stay, PCOA_GRM_SUBSET_PANEL));
        kept.swap(kept_next);
        pruned = false;
      }
    }
    for (int done = 0;;) {
      const int32_t m = (int32_t)kept.size();
      if (conf.grm_ld_window > 0 && !pruned) grm_ld_prune_now(ctx);
      pruned = false;
      check(ctx, pcoa_compute(ctx, conf.num_pc, comps.data(), lam.data(), &nonzero), "computePca");
      if (done == conf.grm_outlier_iterations) break;
      const std::vector<char> removed = outlier_rule(comps.data(), conf.num_pc, m, conf.grm_outlier_sigma);
      std::vector<int32_t> keep, kept_next;
      std::string gone_names;
      for (int32_t a = 0; a < m; ++a) {
        if (removed[(size_t)a]) {
          gone_names += (gone_names.empty() ? ": " : ", ") + names[(size_t)kept[(size_t)a]];
        } else {
          keep.push_back(a);
          kept_next.push_back(kept[(size_t)a]);
        }
      }
      const int32_t gone = m - (int32_t)keep.size();
      std::fprintf(stderr, "Outlier round %d: removed %d sample(s)%s\n", done + 1, gone, gone_names.c_str());
      if (gone == 0) break;
      const int32_t least = std::max(32, conf.num_pc + 1);
      if ((int32_t)keep.size() < least)
        die("--grm-outlier-iterations: round " + std::to_string(done + 1) + " would leave " + std::to_string(keep.size()) + " of " +
            std::to_string(m) + " samples, fewer than the " + std::to_string(least) + " a GRM engine with " + std::to_string(conf.num_pc) +
            " principal components needs; raise --grm-outlier-sigma");
      grm_replace(grm_subset(ctx, m, keep, PCOA_GRM_SUBSET_PANEL));
      kept.swap(kept_next);
      ++done;
    }
  } else if (!strips.empty()) {
    check(ctx, pcoa_compute_strips(owners.data(), (int32_t)owners.size(), conf.num_pc, comps.data(), lam.data(), &nonzero), "computePca");
  } else {
    // --outlier-iterations K: computePca, the rule, and while something is removed and fewer than K rounds have removed
    // something, the engine is replaced by its subset over the kept samples and computePca runs again.  The final cohort
    // always gets a computePca.  K = 0: the one computePca of the reference
    for (int done = 0;;) {
      const int32_t m = (int32_t)kept.size();
      check(ctx, pcoa_compute(ctx, conf.num_pc, comps.data(), lam.data(), &nonzero), "computePca");
      if (done == conf.outlier_iterations) break;
      const std::vector<char> removed = outlier_rule(comps.data(), conf.num_pc, m, conf.outlier_sigma);
      std::vector<int32_t> keep, kept_next;
      std::string gone_names;
      for (int32_t a = 0; a < m; ++a) {
        if (removed[(size_t)a]) {
          gone_names += (gone_names.empty() ? ": " : ", ") + names[(size_t)kept[(size_t)a]];
        } else {
          keep.push_back(a);
          kept_next.push_back(kept[(size_t)a]);
        }
      }
      const int32_t gone = m - (int32_t)keep.size();
      std::fprintf(stderr, "Outlier round %d: removed %d sample(s)%s\n", done + 1, gone, gone_names.c_str());
      if (gone == 0) break;
      const int32_t least = std::max(3, conf.num_pc + 1);
      if ((int32_t)keep.size() < least)
        die("--outlier-iterations: round " + std::to_string(done + 1) + " would leave " + std::to_string(keep.size()) + " of " +
            std::to_string(m) + " samples, fewer than the " + std::to_string(least) + " that " + std::to_string(conf.num_pc) +
            " principal components need; raise --outlier-sigma");
      pcoa_ctx* sub = nullptr;
      check(ctx, pcoa_create_subset(&sub, ctx, keep.data(), (int32_t)keep.size()), "pcoa_create_subset");
      pcoa_timings tp;   // the Gram kernels ran on the predecessor: its time goes into the closing line
      if (pcoa_get_timings(ctx, &tp) == PCOA_OK) gram_s_before += tp.gram_kernel_seconds;
      pcoa_destroy(ctx);
      ctx = owners[0] = sub;
      kept.swap(kept_next);
      ++done;
    }
  }
  const int32_t n_out = (int32_t)kept.size();
  std::printf("Non zero rows in matrix: %d / %d.\n", nonzero, n_out);

  // emitResult (:233-246): the kept samples, in the original order
  std::vector<OutRow> rows;
  for (int32_t a = 0; a < n_out; ++a) {
    const size_t i = (size_t)kept[(size_t)a];
    rows.push_back({names[i], ids[i].substr(0, ids[i].find('-')), comps[(size_t)a], comps[(size_t)a + (size_t)n_out]});
  }
  size_t n_study = 0;
  if (conf.grm && !conf.grm_project_path.empty()) {
    const std::vector<OutRow> study_rows = grm_project_study(conf, ctx, plink, comps, lam, used_stems);
    rows.insert(rows.end(), study_rows.begin(), study_rows.end());
    n_study = study_rows.size();
  }
  std::vector<int32_t> pcr_placed;   // the removed samples --grm-project-removed placed, and their coordinates: --grm-pcrelate-output-path
  std::vector<double> pcr_coords;
  if (conf.grm && conf.grm_project_removed) {
    // every sample of the fileset that is not in the final cohort: one study subset of the ORIGINAL engine on the final axes
    std::vector<int32_t> gone;
    size_t k = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (k < kept.size() && kept[k] == i) ++k;
      else if (conf.grm_project_lsq || !std::binary_search(grm_mind_gone.begin(), grm_mind_gone.end(), i))
        gone.push_back(i);   // (a sparsely called sample is what a mean-imputed projection misplaces: least squares places it)
    }
    if (!gone.empty()) {
      const int32_t nq = (int32_t)gone.size();
      pcoa_ctx* study = grm_subset(grm_full, n, gone, PCOA_GRM_SUBSET_STUDY);
      std::vector<std::string> labels;
      for (int32_t i : gone) labels.push_back(names[(size_t)i]);
      std::vector<double> coords;
      const std::vector<char> placed = grm_place(conf, ctx, study, nq, comps, lam, "removed ", labels, coords);
      pcoa_destroy(study);
      for (int32_t q = 0; q < nq; ++q)
        if (placed[(size_t)q]) pcr_placed.push_back(gone[(size_t)q]);
      pcr_coords.assign((size_t)conf.num_pc * pcr_placed.size(), 0.0);   // [num_pc][placed]
      for (int32_t q = 0, w = 0; q < nq; ++q) {
        if (!placed[(size_t)q]) continue;
        for (int c = 0; c < conf.num_pc; ++c) pcr_coords[(size_t)c * pcr_placed.size() + (size_t)w] = coords[(size_t)q + (size_t)c * (size_t)nq];
        ++w;
      }
      for (int32_t q = 0; q < nq; ++q) {
        if (!placed[(size_t)q]) continue;
        const size_t i = (size_t)gone[(size_t)q];
        rows.push_back({names[i], ids[i].substr(0, ids[i].find('-')), coords[(size_t)q], coords[(size_t)q + (size_t)nq]});
        ++n_study;
      }
    }
  }
  if (conf.grm && conf.has_grm_pcrelate_output_path) {
    // --grm-pcrelate-output-path: the cohort is the final cohort plus the removed samples --grm-project-removed placed, in fileset
    // index order; its engine is the final one, or a panel subset of the whole-fileset engine over the cohort, pruned under
    // --grm-ld-window like every round's engine.  The covariates: a row of ones, then the first K coordinates of every cohort
    // sample (u_c for the final cohort, the projected coordinate for a placed one); the hat matrix is pcoa_pcrelate_hat's.
    // n(i, i) of the inbreeding file comes from pcoa_grm_pcrelate_block's pair counts over diagonal blocks
    const int32_t kp = conf.grm_pcrelate_pcs;
    struct Member { int32_t index; const double* coord; size_t stride; };
    std::vector<Member> cohort;
    for (int32_t a = 0; a < n_out; ++a) cohort.push_back({kept[(size_t)a], comps.data() + a, (size_t)n_out});
    for (size_t q = 0; q < pcr_placed.size(); ++q)
      cohort.push_back({pcr_placed[q], pcr_coords.data() + q, pcr_placed.size()});
    std::stable_sort(cohort.begin(), cohort.end(), [](const Member& x, const Member& y) { return x.index < y.index; });
    const int32_t m = (int32_t)cohort.size();
    pcoa_ctx* eng = ctx;
    pcoa_ctx* sub = nullptr;
    if (!pcr_placed.empty()) {
      const int32_t least = std::max(32, conf.num_pc + 1);
      if (m < least)
        die("--grm-pcrelate-output-path: the cohort holds " + std::to_string(m) + " samples, fewer than the " + std::to_string(least) +
            " a GRM engine with " + std::to_string(conf.num_pc) + " principal components needs");
      std::vector<int32_t> idx;
      for (const Member& mb : cohort) idx.push_back(mb.index);
      sub = grm_subset(grm_full, n, idx, PCOA_GRM_SUBSET_PANEL);
      if (conf.grm_ld_window > 0) grm_ld_prune_now(sub);
      eng = sub;
    }
    std::vector<double> basis((size_t)(kp + 1) * (size_t)m), hat((size_t)(kp + 1) * (size_t)m);
    for (int32_t a = 0; a < m; ++a) {
      basis[(size_t)a] = 1.0;
      for (int32_t c = 0; c < kp; ++c) basis[(size_t)(c + 1) * (size_t)m + (size_t)a] = cohort[(size_t)a].coord[(size_t)c * cohort[(size_t)a].stride];
    }
    if (pcoa_pcrelate_hat(kp + 1, m, basis.data(), hat.data()) != PCOA_OK) die(std::string("pcoa_pcrelate_hat: ") + pcoa_last_error(nullptr));
    check(eng, pcoa_grm_pcrelate_fit(eng, kp + 1, basis.data(), hat.data()), "pcoa_grm_pcrelate_fit");
    std::vector<pcoa_grm_pair> found((size_t)std::min<int64_t>(conf.grm_pcrelate_max_pairs, (int64_t)m * (m - 1) / 2));
    std::vector<double> diag((size_t)m);
    int64_t n_found = 0;
    check(eng, pcoa_grm_pcrelate_pairs(eng, conf.grm_pcrelate_cutoff, conf.grm_pcrelate_maf_threshold, 0, found.empty() ? nullptr : found.data(),
                                       (int64_t)found.size(), &n_found, diag.data()),
          "pcoa_grm_pcrelate_pairs");
    if (n_found > conf.grm_pcrelate_max_pairs)
      die("--grm-pcrelate-cutoff " + java_double(conf.grm_pcrelate_cutoff) + " reports " + std::to_string(n_found) +
          " pairs, more than --grm-pcrelate-max-pairs " + std::to_string(conf.grm_pcrelate_max_pairs) +
          " takes; raise --grm-pcrelate-max-pairs or the cutoff");
    {
      std::ofstream out(conf.grm_pcrelate_output_path);
      out << "name_i\tname_j\tkinship\tn\n";
      for (int64_t e = 0; e < n_found; ++e) {
        const pcoa_grm_pair& p = found[(size_t)e];
        out << names[(size_t)cohort[(size_t)p.i].index] << "\t" << names[(size_t)cohort[(size_t)p.j].index] << "\t" << java_double(p.k) << "\t"
            << p.n << "\n";
      }
      if (!out) die("cannot write " + conf.grm_pcrelate_output_path);
    }
    if (conf.has_grm_pcrelate_inbreeding_output_path) {
      std::vector<int32_t> n_diag((size_t)m), blk;
      for (int32_t r0 = 0; r0 < m; r0 += 1024) {
        const int32_t r = std::min(1024, m - r0);
        blk.assign((size_t)r * (size_t)r, 0);
        check(eng, pcoa_grm_pcrelate_block(eng, r0, r, r0, r, conf.grm_pcrelate_maf_threshold, nullptr, blk.data(), 0), "pcoa_grm_pcrelate_block");
        for (int32_t a = 0; a < r; ++a) n_diag[(size_t)(r0 + a)] = blk[(size_t)a * (size_t)r + (size_t)a];
      }
      std::ofstream out(conf.grm_pcrelate_inbreeding_output_path);
      out << "name\tf\tn\n";
      for (int32_t a = 0; a < m; ++a) {
        const double twice = 2.0 * diag[(size_t)a];
        out << names[(size_t)cohort[(size_t)a].index] << "\t" << java_double(twice - 1.0) << "\t" << n_diag[(size_t)a] << "\n";
      }
      if (!out) die("cannot write " + conf.grm_pcrelate_inbreeding_output_path);
    }
    int64_t used_now = 0;
    if (pcoa_grm_info(eng, nullptr, &used_now, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(eng));
    std::fprintf(stderr, "GRM PC-Relate: %lld pair(s) with kinship >= %s among %d sample(s), %d %s, %lld used variant(s), threshold %s\n",
                 (long long)n_found, java_double(conf.grm_pcrelate_cutoff).c_str(), m, kp, kp == 1 ? "axis" : "axes", (long long)used_now,
                 java_double(conf.grm_pcrelate_maf_threshold).c_str());
    if (sub) pcoa_destroy(sub);
  }
  if (conf.grm && conf.grm_project_removed && grm_full != ctx) pcoa_destroy(grm_full);
  emit_result(conf, rows, n_study);

  // --grm-weights-output-path: the left singular vectors of the standardised genotype matrix, one line per variant of the store
  if (conf.grm && !conf.grm_weights_output_path.empty()) {
    int64_t n_rows = 0;
    if (pcoa_grm_info(ctx, &n_rows, nullptr, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(ctx));
    if ((int64_t)fed_meta.size() != n_rows)
      die("--grm-weights-output-path: " + std::to_string(fed_meta.size()) + " variant records for " + std::to_string(n_rows) + " rows");
    std::vector<double> w((size_t)std::max<int64_t>(n_rows, 1) * (size_t)conf.num_pc);
    check(ctx, pcoa_grm_weights(ctx, conf.num_pc, comps.data(), lam.data(), 1, 0, n_rows, w.data()), "pcoa_grm_weights");
    std::ofstream out(conf.grm_weights_output_path);
    for (int64_t v = 0; v < n_rows; ++v) {
      out << v << "\t" << fed_meta[(size_t)v].contig << "\t" << fed_meta[(size_t)v].pos << "\t" << fed_meta[(size_t)v].id;
      for (int c = 0; c < conf.num_pc; ++c) out << "\t" << java_double(w[(size_t)v * (size_t)conf.num_pc + (size_t)c]);
      out << "\n";
    }
    if (!out) die("cannot write " + conf.grm_weights_output_path);
  }

  // --grm-output-path: K out of the engine in bands of 1,024 rows, columns 0 .. band end (pcoa_grm_block, host pointers): no
  // N x N array exists on either side.  Rows are the samples in the engine's index order; the float32 cast is the language's own
  if (conf.grm && !conf.grm_output_path.empty()) {
    const int32_t divisor = conf.grm_output_divisor == "pairwise" ? PCOA_GRM_DIVISOR_PAIRWISE : PCOA_GRM_DIVISOR_USED;
    const int32_t band = 1024;
    std::ofstream fk(conf.grm_output_path + ".grm.bin", std::ios::binary), fn(conf.grm_output_path + ".grm.N.bin", std::ios::binary);
    std::vector<double> kb;
    std::vector<int32_t> nb;
    std::vector<float> line;
    long long written = 0;
    for (int32_t r0 = 0; r0 < n_out; r0 += band) {
      const int32_t r = std::min(band, n_out - r0), cols = r0 + r;
      kb.resize((size_t)r * (size_t)cols);
      nb.resize((size_t)r * (size_t)cols);
      check(ctx, pcoa_grm_block(ctx, r0, r, 0, cols, divisor, kb.data(), nb.data(), 0), "pcoa_grm_block");
      for (int32_t a = 0; a < r; ++a) {
        const size_t len = (size_t)(r0 + a) + 1;
        line.resize(len);
        for (size_t j = 0; j < len; ++j) line[j] = (float)kb[(size_t)a * (size_t)cols + j];
        fk.write(reinterpret_cast<const char*>(line.data()), (std::streamsize)(len * sizeof(float)));
        for (size_t j = 0; j < len; ++j) line[j] = (float)nb[(size_t)a * (size_t)cols + j];
        fn.write(reinterpret_cast<const char*>(line.data()), (std::streamsize)(len * sizeof(float)));
        written += 2 * (long long)(len * sizeof(float));
      }
    }
    std::ofstream fi(conf.grm_output_path + ".grm.id");
    for (int32_t a = 0; a < n_out; ++a) {   // the final cohort's samples, in the engine's index order
      const size_t i = (size_t)kept[(size_t)a];
      fi << ids[i].substr(0, ids[i].find('-')) << "\t" << names[i] << "\n";
    }
    if (!fk || !fn || !fi) die("cannot write " + conf.grm_output_path + ".grm.*");
    int64_t used = 0;
    if (pcoa_grm_info(ctx, nullptr, &used, nullptr) != 1) die(std::string("pcoa_grm_info: ") + pcoa_last_error(ctx));
    std::fprintf(stderr, "GRM written: %d samples, %lld used variants, divisor %s, %lld bytes\n", n_out, (long long)used,
                 divisor == PCOA_GRM_DIVISOR_PAIRWISE ? "pairwise" : "used", written);
  }

  // --loadings-output-path: w_c = X (J u_c) / sqrt(lambda_c) for every variant the engine was fed, from the eigenpairs above
  if (want_loadings) {
    std::vector<double> w;
    int64_t n_rows = 0;
    check(ctx, pcoa_loadings_begin(ctx, conf.num_pc, comps.data(), lam.data(), PCOA_LOADINGS_CENTRE | PCOA_LOADINGS_UNIT), "loadings");
    if (conf.gram == "implicit") {   // the rows are the engine's own store
      (void)pcoa_operator_info(ctx, &n_rows, nullptr);
      w.resize((size_t)std::max<int64_t>(n_rows, 1) * (size_t)conf.num_pc);
      check(ctx, pcoa_loadings_operator(ctx, 0, n_rows, w.data(), 0), "loadings");
    } else {
      // stored S: the .bed a second time, block by block through the page-locked blocks of the first pass -- block k + 1 is read
      // while block k's rows are decoded and summed on the device (a host `out` is filled when the call returns)
      n_rows = (int64_t)std::count(plink.keep.begin(), plink.keep.end(), (char)1);
      w.resize((size_t)std::max<int64_t>(n_rows, 1) * (size_t)conf.num_pc);
      const int fd = ::open((plink.prefix + ".bed").c_str(), O_RDONLY);
      if (fd < 0) die("cannot open " + plink.prefix + ".bed");
      const int64_t total = (int64_t)plink.keep.size(), block = conf.stream_rows;
      const size_t bpv = plink.bpv;
      auto read_block = [&](int64_t b0, int which) -> int64_t {   // kept rows, compacted to the front of blocks[which]
        const int64_t nrows = std::min(block, total - b0);
        unsigned char* dst = blocks[(size_t)which];
        size_t lo = 0;
        const size_t hi = (size_t)nrows * bpv;
        while (lo < hi) {
          const ssize_t r = ::pread(fd, dst + lo, hi - lo, (off_t)(3 + (size_t)b0 * bpv + lo));
          if (r <= 0) die(plink.prefix + ".bed: read error");
          lo += (size_t)r;
        }
        int64_t kept_rows = 0;
        for (int64_t r = 0; r < nrows; ++r) {
          if (!plink.keep[(size_t)(b0 + r)]) continue;
          if (kept_rows != r) std::memmove(dst + (size_t)kept_rows * bpv, dst + (size_t)r * bpv, bpv);
          ++kept_rows;
        }
        return kept_rows;
      };
      int which = 0;
      int64_t done = 0;
      int64_t kept_rows = total > 0 ? read_block(0, 0) : 0;
      for (int64_t b0 = 0; b0 < total; b0 += block) {
        std::future<int64_t> next;
        if (b0 + block < total) next = std::async(std::launch::async, read_block, b0 + block, (which + 1) & 3);
        if (kept_rows > 0)
          check(ctx, pcoa_loadings_plink_bed(ctx, blocks[(size_t)which], kept_rows, (int64_t)bpv, conf.plink_ref_allele == "a1" ? 1 : 0, 0,
                                             w.data() + (size_t)done * (size_t)conf.num_pc, 0), "loadings");
        done += kept_rows;
        if (next.valid()) kept_rows = next.get();
        which = (which + 1) & 3;
      }
      ::close(fd);
      if (done != n_rows) die("--loadings-output-path: the second pass read " + std::to_string(done) + " rows, the first " + std::to_string(n_rows));
    }
    check(ctx, pcoa_loadings_end(ctx), "loadings");
    if (fed_meta_known && (int64_t)fed_meta.size() != n_rows)
      die("--loadings-output-path: " + std::to_string(fed_meta.size()) + " variant records for " + std::to_string(n_rows) + " rows");
    std::ofstream out(conf.loadings_output_path);
    for (int64_t v = 0; v < n_rows; ++v) {
      if (fed_meta_known) out << v << "\t" << fed_meta[(size_t)v].contig << "\t" << fed_meta[(size_t)v].pos << "\t" << fed_meta[(size_t)v].id;
      else out << v << "\t.\t.\t.";
      for (int c = 0; c < conf.num_pc; ++c) out << "\t" << java_double(w[(size_t)v * (size_t)conf.num_pc + (size_t)c]);
      out << "\n";
    }
    if (!out) die("cannot write " + conf.loadings_output_path);
  }
  for (unsigned char* b : blocks) (void)pcoa_host_free_pinned(b);

  // reportIoStats (:48) / stop (:49)
  pcoa_timings t;
  if (pcoa_get_timings(ctx, &t) == PCOA_OK) {
    double gram_s = t.gram_kernel_seconds + gram_s_before;   // (strip layout: summed over the owners)
    for (size_t g = 1; g < owners.size(); ++g) {
      pcoa_timings tg;
      if (pcoa_get_timings(owners[g], &tg) == PCOA_OK) gram_s += tg.gram_kernel_seconds;
    }
    std::fprintf(stderr, "Variants accumulated: %lld; Gram kernel %.3f ms; PCoA %.3f ms\n", (long long)t.gram_variants,
                 1e3 * gram_s, 1e3 * t.compute_total_seconds);
    int64_t op_variants = 0, op_bytes = 0;
    if (pcoa_operator_info(ctx, &op_variants, &op_bytes) == 1)
      std::fprintf(stderr, "Implicit similarity operator: %lld variants in %.1f MB of carrier bitsets, %d Lanczos steps over S v = X^T (X v)\n",
                   (long long)op_variants, op_bytes / 1e6, t.lanczos_steps);
    if (!strips.empty())
      std::fprintf(stderr, "computePca over %zu strip owners: %d Lanczos steps (each one product over every owner)\n", owners.size(),
                   t.lanczos_steps);
  }
  for (pcoa_ctx* o : owners) pcoa_destroy(o);
  if (g_calls.companion) pcoa_destroy(g_calls.companion);   // (after the engine it was bound to)
  return 0;
}
