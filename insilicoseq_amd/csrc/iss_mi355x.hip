// iss_mi355x.hip -- C-ABI shared library of the MI355X read-generation engine (see include/iss_mi355x.h).
// Host side: context, HBM uploads (model tables, genomes; small records from an arena), launch sequencing on one HIP
// stream for one record (iss_generate) or a whole work list (iss_generate_batch: records side by side in one arena),
// HIP-event timing, downloads, the FASTQ pipeline (text or gzip members built on the device, copy stream, writer thread) and the
// append pipe of the one-file outputs (VCF text, unaligned BAM, origins text: iss_host_pipe.hip.h).
// Device side: iss_kernels.hip.h (the Philox path), iss_perfect.hip.h (its perfect-model kernel), iss_mt_compat.hip.h (the reference's Mersenne-Twister streams),
// iss_fastq.hip.h, iss_deflate.hip.h, iss_vcf.hip.h (the --store_mutations text); `model` (BAM tallies, KDE): iss_bam.hip.h;
// iss_export.hip.h (the rows as dense device arrays for a consumer on the GPU), iss_truth.hip.h (their mutation rows likewise),
// iss_tally.hip.h (integer tallies of the rows: what a run produced), iss_depth.hip.h (per-base coverage depth of the reads),
// iss_ubam.hip.h (the rows as unaligned BAM: records and BGZF members), iss_origins.hip.h (every pair's source intervals as BEDPE text),
// iss_bgzf_text.hip.h (the VCF and origins text as BGZF members), iss_errtally.hip.h (integer tallies of the mutation rows: what
// a run did to the reads), iss_fqtally.hip.h (`report`: the tallies of iss_tally.hip.h over FASTQ text), iss_inflate.hip.h (BGZF
// members inflated: the decoder of iss_inflate_core.h on 64 lanes), iss_bamreads.hip.h (`report --bam`: the same tallies over BAM records),
// iss_variants.hip.h (`generate --variants`: a VCF's alleles spliced into a record, coordinates lifted back; the mapping: iss_variants_core.h),
// iss_fasta.hip.h (`generate --device_fasta`: the genome FASTA indexed and its line ends removed; the grammar: iss_fasta_core.h).
#include "iss_mi355x.h"

#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "iss_kernels.hip.h"
#include "iss_perfect.hip.h"     // k_perfect: quality mode 2 (PerfectErrorModel)
#include "iss_pack_group.hip.h"  // k_pack_group: records uploaded in groups (draft contigs)
#include "iss_fastq.hip.h"
#include "iss_deflate.hip.h"
#include "iss_mt_compat.hip.h"
#include "iss_units.hip.h"
#include "iss_bam.hip.h"        // `model`: BAM tallies and the KDE CDFs
#include "iss_vcf.hip.h"        // --store_mutations: the VCF text (last: the kernels before it keep their places in the code object)
#include "iss_export.hip.h"     // k_rows_export: the rows as dense arrays in the caller's device memory (behind every other kernel, for the same reason)
#include "iss_truth.hip.h"      // k_truth_scatter, k_truth_events: the mutation rows as dense device arrays (behind those again)
#include "iss_tally.hip.h"      // k_tally_lines, k_tally_reads: quality, base, GC and insert-size tallies of the rows (last, likewise)
#include "iss_depth.hip.h"      // k_depth_*: per-base coverage depth of the reads (behind every other kernel, likewise)
#include "iss_ubam.hip.h"       // k_ubam_format, k_bgzf_*: unaligned BAM records and their BGZF members (last, likewise)
#include "iss_origins.hip.h"    // k_origins_len, k_origins_format: the pairs' source intervals as BEDPE text (last, likewise)
#include "iss_bgzf_text.hip.h"  // k_bgzt_*: the VCF and origins text as BGZF members, copies from the line above (last, likewise)
#include "iss_errtally.hip.h"   // k_errtally_rows, k_errtally_reads: tallies of the mutation rows (last, likewise)
#include "iss_fqtally.hip.h"    // k_fq_*: `report`, the tallies of the rows over FASTQ text (last, likewise)
#include "iss_inflate.hip.h"    // k_bgzf_inflate: BGZF members inflated on the device (last, likewise)
#include "iss_bamreads.hip.h"   // k_br_*: `report --bam`, the tallies of k_fq_* over BAM records (last, likewise)
#include "iss_bamerrors.hip.h"  // k_be_*: `report --bam --errors`, the errors CIGAR and MD tell of (last, likewise)
#include "iss_bamdepth.hip.h"   // k_bd_records: `report --bam --depth`, the reference intervals the CIGARs cover (last, likewise)
#include "iss_variants.hip.h"   // k_variant_*: `generate --variants`, a record's haplotype spliced in front of k_pack_genome (last, likewise)
#include "iss_fasta.hip.h"      // k_fa_*: `generate --device_fasta`, a FASTA text indexed and stripped in front of the pack kernels (last, likewise)

// The host side by concern (one translation unit, one shared library; the order is the order of definition):
#include "iss_own.h"                  // the owning handle (plain C++: device and pinned memory, events, streams)
#include "iss_host_state.hip.h"       // the output pipes' records, struct iss_ctx
#include "iss_host_util.hip.h"        // errors, checked allocations and uploads, switches, kernel choice, timing, synchronisation
#include "iss_host_session.hip.h"     // shared by the stand-alone contexts (iss_bam, iss_fq, iss_inflate, iss_br): open and close, slots, grown buffers
#include "iss_host_mt_streams.hip.h"  // MT19937 seeding and fill launches
#include "iss_host_pipe.hip.h"        // shared by the output pipes: slot table, slot wait, the append pipe and its writer thread
#include "iss_host_fastq_pipe.hip.h"  // the two FASTQ files' writer thread, flush
#include "iss_host_bgzf_text.hip.h"   // the BGZF stage of the two text pipes: buffers, launches, the members' check and write
#include "iss_host_vcf_pipe.hip.h"    // append pipe: the VCF text's check and write
#include "iss_host_ubam_pipe.hip.h"   // append pipe: the BGZF members' check and write
#include "iss_host_origins_pipe.hip.h"  // append pipe: the origins text's write
#include "iss_api_context.hip.h"
#include "iss_api_model.hip.h"
#include "iss_api_generate.hip.h"
#include "iss_api_mt.hip.h"
#include "iss_api_fastq.hip.h"
#include "iss_api_vcf.hip.h"
#include "iss_api_bam.hip.h"
#include "iss_api_export.hip.h"
#include "iss_api_tally.hip.h"
#include "iss_api_depth.hip.h"
#include "iss_api_ubam.hip.h"
#include "iss_api_origins.hip.h"
#include "iss_api_errtally.hip.h"
#include "iss_api_fqtally.hip.h"
#include "iss_api_inflate.hip.h"
#include "iss_api_bamreads.hip.h"
#include "iss_api_variants.hip.h"
#include "iss_api_fasta.hip.h"
