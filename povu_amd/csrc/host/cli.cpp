// cli.cpp -- the `povu` command line for the decompose path.
// Same surface as the reference for this path (app/cli/cli.cpp:14-26,236-262,324-382, app/main.cpp):
//   povu [--version] [-v <int>] [-t <int>] decompose -i <gfa> [-o <dir>] [-h|--hairpins] [-s|--subflubbles]
//   povu ... decompose ... --structure-export <json>   (additive: writes the flubble debug sidecar gfa2vcf writes)
//   povu ... gfa2vcf -i <gfa> [-h] [-s] [--structure-export <json>] <options of `call`>   (app/cli/cli.cpp:154-193)
//   povu ... call -i <gfa> [-f <dir>] (-r <file> | -P <prefix>... | <prefix>...) [-o <dir> | --stdout] [--inversions] [--nested] [--spanning-alleles] [--profile <p>] [--merge-primitives] [--off-reference] [--untangle] [--region <name:start-end>]... [--cluster <F>]   (the
//   variant calls of INTEGRATION.md "Variant calls" and "Inversion calls", on the GPU)
//   povu ... vcf -i <gfa> -c <vcf> --report -o <dir> [--spelling] [--forward-only]   (the --report half of the reference's `vcf`,
//   app/cli/cli.cpp; INTEGRATION.md "VCF checks", on the GPU)
//   povu ... vcf -c <vcf> -d <vcf> --compare -o <dir>   (the reference's flag names, a definition of this project's own:
//   INTEGRATION.md "VCF comparison", on the GPU; -i is accepted and not read)
//   povu ... vcf -c <vcf> -d <vcf> --compare --haplotypes [-i <gfa>] [--max-reach <n>] -o <dir>   (INTEGRATION.md "Haplotype
//   comparison", on the GPU: with -i the GFA's paths are the reference, without it the REF fields are)
//   povu ... vcf -i <gfa> -c <vcf> --consensus [--roundtrip] [--no-fasta] [--sample <name>]... [--chrom <name>]... [--line-width <n>]
//   -o <dir>   (INTEGRATION.md "Consensus haplotypes", on the GPU)
#include "decompose.hpp"

#include <cstdlib>
#include <cxxabi.h>
#include <typeinfo>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

static const char *VERSION = "0.0.1-alpha"; // app/cli/cli.hpp:10

static void usage(std::ostream &os)
{
	os << "  povu {OPTIONS} [COMMAND]\n\n"
	      "    Explore variation in a variation graph\n\n"
	      "  OPTIONS:\n\n"
	      "      commands\n"
	      "        decompose                         Find regions of variation\n"
	      "        info                              Print graph information [uses 1 thread]\n"
	      "        prune                             Reduce GFA to graph structure\n"
	      "        gfa2vcf                           Convert GFA to VCF (decompose here + `call` of $POVU_CALL_EXE)\n"
	      "        call                              Call variants of a forest on the GPU and write VCF\n"
	      "        vcf                               Check a VCF against the graph on the GPU (--report)\n"
	      "      arguments\n"
	      "        --version                         The current version of povu\n"
	      "        -v[verbosity],\n"
	      "        --verbosity=[verbosity]           Level of output [default: 0]\n"
	      "        -t[threads], --threads=[threads]  Number of threads to use [default: 1]\n"
	      "        -h, --help                        help\n\n"
	      "  decompose OPTIONS:\n"
	      "        -i[gfa], --input-gfa=[gfa]        path to input gfa [required]\n"
	      "        -o[output_dir],\n"
	      "        --output-dir=[output_dir]         Output directory [default: .]\n"
	      "        -h, --hairpins                    Find hairpins in the variation graph [default: false]\n"
	      "        -s, --subflubbles                 Find subflubbles in the variation graph [default: false]\n"
	      "                                          (tiny, parallel, concealed, midi and smothered: T O C M S lines)\n"
	      "        --leaf-subflubbles                Relabel leaf flubbles as tiny (T) / parallel (O): the find_tiny and\n"
	      "                                          find_parallel passes of -s, without its three inserting passes\n"
	      "        --traversals                      Also write <component id>.trav: the traversals of every flubble by the\n"
	      "                                          GFA's P / W paths and their alleles (one GPU only)\n"
	      "        --gpus=[n]                        Shard the components over n GPUs of this node, one worker per GPU\n"
	      "                                          [default: 1; devices 0..n-1 or $POVU_HIP_DEVICES]\n"
	      "        --structure-export=[structure_json]\n"
	      "                                          Write the flubble debug sidecar <structure_json>.flubble-debug.jsonl\n"
	      "                                          [conformance]\n\n"
	      "  call OPTIONS:\n"
	      "        -i[gfa], --input-gfa=[gfa]        path to input gfa [required]\n"
	      "        -f[forest_dir], --forest-dir=[forest_dir]\n"
	      "                                          directory of the <component id>.pvst files [default: .]\n"
	      "        -r[ref_list], --ref-list=[ref_list]\n"
	      "                                          file of reference path name prefixes, one per line\n"
	      "        -P[prefix], --path-prefix=[prefix]\n"
	      "                                          reference paths: every path whose name starts with it (repeatable)\n"
	      "        prefixes...                       reference path name prefixes (exactly one of -r, -P, positional)\n"
	      "        -o[output_dir], --output-dir=[output_dir]\n"
	      "                                          write <output_dir>/<prefix>.vcf per prefix\n"
	      "        --stdout                          one VCF of every reference path to stdout [default]\n"
	      "        --inversions                      also call inversions: a VARTYPE=SUBR record for every stretch of two or more\n"
	      "                                          steps of a reference path that another path walks backwards [default: false]\n"
	      "        --nested                          alleles modulo enclosed sites, LV and PS by the nesting of traversals\n"
	      "                                          (INTEGRATION.md \"Nested calls\") [default: false]\n"
	      "        --spanning-alleles                nested calls only: a '*' ALT, last, for the haplotypes that cross an enclosing site\n"
	      "                                          on an allele without this one, instead of '.' (INTEGRATION.md \"Spanning alleles\");\n"
	      "                                          not with the left-normalized and decomposed profiles [default: false]\n"
	      "        --profile=[raw-graph|top-level-only|popped|left-normalized]\n"
	      "                                          which records to keep (top-level-only and popped imply --nested); left-normalized\n"
	      "                                          keeps all and moves every indel to the left end of its repeat [default: raw-graph]\n"
	      "        --profile=decomposed              keeps all and writes every (REF, ALT) as the SNPs, insertions and deletions of\n"
	      "                                          its alignment (INTEGRATION.md \"Decomposed calls\")\n"
	      "        --merge-primitives                decomposed only: equal primitives of different ALTs and records become one\n"
	      "                                          record with joint genotypes (INTEGRATION.md \"Merged primitives\") [default: false]\n"
	      "        --off-reference                   raw-graph only: also call the sites no reference path crosses, on the first path\n"
	      "                                          that traverses them (INTEGRATION.md \"Off-reference calls\"); with -o the records\n"
	      "                                          no prefix takes go to <output_dir>/off-reference.vcf [default: false]\n"
	      "        --untangle                        raw-graph only: where a haplotype walks a site more than once, align its laps with\n"
	      "                                          the reference's and genotype every copy on its own: LN, LC and GT:CN\n"
	      "                                          (INTEGRATION.md \"Untangled calls\") [default: false]\n"
	      "        --region=[name:start-end]         only the records of the sites with a boundary segment, and of the inversions with an\n"
	      "                                          end step, in the bases [start, end) of the path named exactly so: 1-based start,\n"
	      "                                          exclusive end; repeatable, any path (INTEGRATION.md \"Region calls\"); not with\n"
	      "                                          --off-reference.  (-g / --restrict of the reference tool stay refused)\n"
	      "        --cluster=[F]                     raw-graph only: the exact alleles of a site whose inner segments are similar\n"
	      "                                          (weighted Jaccard of at least F, 0 < F <= 1, at most six decimals) become one\n"
	      "                                          allele, written as its first member, with NX and MINSIM (INTEGRATION.md\n"
	      "                                          \"Clustered calls\"); with --inversions and --region alone [default: off]\n"
	      "        --max-level=[n]                   popped: the deepest level kept without rescue [default: 0]\n"
	      "        --max-ref-length=[n], --max-allele-length=[n]\n"
	      "                                          popped: a record with a longer REF / allele is big (0: no limit) [default: 0]\n"
	      "                                          decomposed: --max-allele-length is the longest allele that is aligned, a longer\n"
	      "                                          one is kept whole (0: 512, the most) [default: 0]\n"
	      "        -c, -q                            accepted and ignored (no streaming here)\n\n"
	      "  vcf OPTIONS:\n"
	      "        -i[gfa], --input-gfa=[gfa]        path to input gfa [required]\n"
	      "        -c[vcf], --vcf=[vcf]              path to the VCF to check [required]\n"
	      "        --report                          check every called allele's AT walk against the paths of its haplotype\n"
	      "                                          and write report.tsv and summary.txt [required: --tui is not provided]\n"
	      "        -o[output_dir], --output-dir=[output_dir]\n"
	      "                                          Output directory [default: .]\n"
	      "        --spelling                        also compare REF and ALT with the sequences of their walks (raw-graph\n"
	      "                                          output; rewritten records fail it) [default: false]\n"
	      "        --forward-only                    the reference's literal rule: a walk found only reversed is absent\n"
	      "                                          [default: false]\n"
	      "        --compare                         instead of --report: compare the alleles and genotypes of -c (side A) with those\n"
	      "                                          of -d (side B) by CHROM, POS, REF and ALT after trimming, and write compare.tsv\n"
	      "                                          and summary.txt; -i is accepted and not read [default: false]\n"
	      "        -d[vcf], --other-input-vcf=[vcf]  path to the other VCF [required by --compare]\n"
	      "        --haplotypes                      with --compare: also compare, per region, sample and phase, the bases the two VCFs\n"
	      "                                          spell, and write haplotypes.tsv and hap_summary.txt; with -i the GFA's paths are\n"
	      "                                          the reference, without it the REF fields are [default: false]\n"
	      "        --max-reach=[n]                   with --haplotypes and -i: bases an indel may reach through its repeat in either\n"
	      "                                          direction, 0 to 65536 [default: 256]\n"
	      "        --consensus                       instead of --report: apply the calls of -c to the paths of -i their CHROMs name and\n"
	      "                                          write consensus.fa (a record per sample, phase and CHROM), roundtrip.tsv and\n"
	      "                                          cons_summary.txt [default: false]\n"
	      "        --roundtrip                       with --consensus: compare every haplotype with the path of its sample and phase\n"
	      "        --no-fasta                        with --consensus: lengths, counts and the round trip only, no consensus.fa\n"
	      "        --sample=[name]...                with --consensus: only these sample columns\n"
	      "        --chrom=[name]...                 with --consensus: only these CHROMs\n"
	      "        --line-width=[n]                  with --consensus: bases a line of consensus.fa, 0 for no wrap [default: 60]\n";
}

int main(int argc, char **argv)
{
	povu_host::Config cfg;
	std::string command;
	bool version = false, help = false, have_input = false, print_tips = false;
	std::vector<std::string> call_args; // gfa2vcf: everything that belongs to `call`
	auto value = [&](int &i, const char *a, const char *shortf, const char *longf, std::string &out) -> bool {
		const size_t ls = strlen(shortf), ll = strlen(longf);
		if (!strncmp(a, longf, ll) && a[ll] == '=') {
			out = a + ll + 1;
			return true;
		}
		if (!strcmp(a, longf) || !strcmp(a, shortf)) {
			if (i + 1 >= argc) {
				std::cerr << "Flag '" << a << "' requires an argument but received none" << std::endl;
				usage(std::cerr);
				std::exit(1);
			}
			out = argv[++i];
			return true;
		}
		if (!strncmp(a, shortf, ls) && a[ls] && a[1] != '-') {
			out = a + ls;
			return true;
		}
		return false;
	};
	for (int i = 1; i < argc; i++) {
		const char *a = argv[i];
		std::string v;
		if (!strcmp(a, "--version")) {
			version = true;
		} else if (!strcmp(a, "--help") || (!strcmp(a, "-h") && command.empty())) {
			help = true;
		} else if (value(i, a, "-v", "--verbosity", v)) {
			cfg.verbosity = atoi(v.c_str());
		} else if (command == "info" && (!strcmp(a, "-t") || !strcmp(a, "--print_tips"))) {
			print_tips = true; // inside `info`, -t means "print the tips" (cli.cpp:220)
		} else if (value(i, a, "-t", "--threads", v)) {
			cfg.threads = atoi(v.c_str());
		} else if ((command == "decompose" || command == "info" || command == "prune" || command == "gfa2vcf" || command == "call" || command == "vcf") &&
			   value(i, a, "-i", "--input-gfa", v)) {
			cfg.input_gfa = v;
			have_input = true;
		} else if ((command == "decompose" || command == "prune") && value(i, a, "-o", "--output-dir", v)) {
			cfg.output_dir = v;
		} else if ((command == "decompose" || command == "gfa2vcf") && (!strcmp(a, "-h") || !strcmp(a, "--hairpins"))) {
			cfg.hairpins = true;
		} else if ((command == "decompose" || command == "gfa2vcf") && (!strcmp(a, "-s") || !strcmp(a, "--subflubbles"))) {
			cfg.subflubbles = true;
		} else if ((command == "decompose" || command == "gfa2vcf") && !strcmp(a, "--leaf-subflubbles")) {
			cfg.leaf_subflubbles = true;
		} else if (command == "decompose" && !strcmp(a, "--traversals")) {
			cfg.traversals = true;
		} else if (command == "decompose" && value(i, a, "--gpus", "--gpus", v)) {
			cfg.gpus = atoi(v.c_str());
			if (cfg.gpus < 1 || cfg.gpus > 64) {
				std::cerr << "Flag '--gpus' expects a number of GPUs between 1 and 64" << std::endl;
				return 1;
			}
		} else if ((command == "decompose" || command == "gfa2vcf") && !strncmp(a, "--structure-export", 18) &&
			   (a[18] == 0 || a[18] == '=')) {
			if (a[18] == '=') {
				cfg.structure_export = a + 19;
			} else if (i + 1 < argc) {
				cfg.structure_export = argv[++i];
			} else {
				std::cerr << "Flag '" << a << "' requires an argument but received none" << std::endl;
				usage(std::cerr);
				return 1;
			}
		} else if (command == "gfa2vcf" || command == "call" || command == "vcf") {
			call_args.push_back(a); // streaming / output / reference options of `call` (cli.cpp:28-88)
		} else if (command.empty() && a[0] != '-') {
			command = a;
		} else {
			if (!version) {
				std::cerr << "Flag could not be matched: " << a << std::endl;
				usage(std::cerr);
				return 1;
			}
		}
	}
	if (cfg.traversals && cfg.gpus > 1) { // (the traversals need a forest of the whole resident graph: sharded ones are refused)
		std::cerr << "Flag '--traversals' cannot be combined with '--gpus' above 1" << std::endl;
		return 1;
	}
	if (version) {
		std::cout << VERSION << std::endl;
		return EXIT_SUCCESS;
	}
	if (help || command.empty()) {
		usage(std::cout);
		return 0;
	}
	if (command != "decompose" && command != "info" && command != "prune" && command != "gfa2vcf" && command != "call" && command != "vcf") {
		std::cerr << "povu (MI355X build): only `decompose`, `info`, `prune`, `gfa2vcf`, `call` and `vcf` are provided; `" << command
			  << "` belongs to the reference CPU tool" << std::endl;
		return 1;
	}
	if (!have_input && !(command == "vcf" && povu_host::vcf_args_check_gfa_themselves(call_args))) {
		std::cerr << "Flag 'gfa' is required" << std::endl;
		usage(std::cerr);
		return 1;
	}
	if (const char *d = std::getenv("POVU_HIP_DEVICE"))
		cfg.device = atoi(d);
	// The reference lets exceptions escape main (uncaught -> std::terminate -> abort).  Same message, same non-zero exit,
	// but an orderly one: this process holds a GPU context, and an abort would take it down mid-flight.
	try {
		if (command == "info")
			povu_host::do_info(cfg, print_tips);
		else if (command == "prune")
			povu_host::do_prune(cfg);
		else if (command == "gfa2vcf")
			povu_host::do_gfa2vcf(cfg, call_args);
		else if (command == "call")
			povu_host::do_call(cfg, call_args);
		else if (command == "vcf")
			povu_host::do_vcf(cfg, call_args);
		else {
			povu_host::reset_debug_sidecar(cfg);
			cfg.exit_when_done = true;
			povu_host::do_decompose(cfg);
		}
	} catch (const std::exception &e) {
		// (the line libstdc++'s terminate handler prints, with the exception's real dynamic type; the exit code is 1 where the
		// reference's abort gives 134 -- documented in DESIGN.md section 1)
		int status = 0;
		char *name = abi::__cxa_demangle(typeid(e).name(), nullptr, nullptr, &status);
		std::cerr << "terminate called after throwing an instance of '" << (status == 0 && name ? name : typeid(e).name())
			  << "'\n  what():  " << e.what() << std::endl;
		free(name);
		return EXIT_FAILURE;
	}
	return 0;
}
