// stride_main.cpp -- `stride pbcorrect` (a.k.a. PacBioSelfCorrection), `stride index`, `stride merge`, `stride sai`,
// `stride grep`, `stride filter`, `stride correct`, `stride fmwalk`, `stride overlap` and `stride fm-merge` on the MI355X back end.  Option surface, defaults, validation messages and exit codes follow the reference's
// StriDe/PacBioSelfCorrection.cpp:32-140,262-434 and StriDe/StriDe.cpp:62-126; extra flags: --devices, --batch.
#include <getopt.h>

#include <array>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lrsc.h"
#include "BCode.h"
#include "ErrorCorrectProcess.h"
#include "FMIndexWalkProcess.h"
#include "FMMergeProcess.h"
#include "KmerDistribution.h"
#include "LexicoOrder.h"
#include "OverlapProcess.h"
#include "PacBioSelfCorrectionProcess.h"
#include "QCProcess.h"
#include "SequenceProcessFramework.h"

#define PACKAGE_NAME "StriDe"
#define PACKAGE_VERSION "0.0.1"
#define PACKAGE_BUGREPORT "ythuang@cs.ccu.edu.tw"
#define SUBPROGRAM "PacBioSelfCorrection"
#define BWT_EXT ".bwt"
#define RBWT_EXT ".rbwt"

using namespace stride;
namespace stride {
int kmerfreqMain(int argc, char** argv);       // tools.cpp
int kmercheckMain(int argc, char** argv);
}

static const char* CORRECT_VERSION_MESSAGE = SUBPROGRAM " Version " PACKAGE_VERSION " (MI355X back end)\n";

static const char* CORRECT_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " " SUBPROGRAM " [OPTION] ... READSFILE\n"
    "Correct PacBio reads via FM-index walk\n"
    "\n"
    "      -t, --thread=NUM                 Use NUM threads for the computation (default: 1)\n"
    "      -p, --prefix=PREFIX              Use PREFIX for the names of the index files\n"
    "      --build-index                    Index READSFILE in memory on the first device instead of loading PREFIX.bwt/.rbwt\n"
    "      --save-index=PREFIX              With --build-index: write the built index to PREFIX.bwt/.rbwt/.sai/.rsai\n"
    "      --merge-index=PREFIX             With --build-index: correct against the index of PREFIX's reads followed by READSFILE's,\n"
    "                                       merged on the first device from PREFIX.bwt/.rbwt and the built index\n"
    "      --load-on-device                 With -p: decode PREFIX.bwt/.rbwt on the first device instead of on the host\n"
    "      -o, --output=DIR                 Output results in the directory\n"
    "      -b, --barcode=FILE               Barcode of raw reads\n"
    "\nPacBio correction parameters:\n"
    "      -c, --PBcoverage=N               Coverage of PacBio reads (default: 90)\n"
    "      -e, --error-rate=N               The error rate of PacBio reads.(default:0.15)\n"
    "      -k, --kmer-size=N                The start kmer length (default: 19 (PacBioS).)\n"
    "      -n, --next-target                The number of next FMWalk target seed(default: 1)\n"
    "      -l, --max-leaves=N               Number of maximum leaves in the search tree. (default: 32)\n"
    "      -i, --idmer-length=N             The length of the kmer to identify similar reads.(default: 9)\n"
    "      -s, --min-kmer-size=N            The minimum length of the kmer to use. (default: 13.)\n"
    "      -g, --genome=(5/10/100)[m]       Genome size of the species (default: 10m)\n"
    "      -m, --mode=(0/1/2)               Mode in seed-searching (default: 1)\n"
    "      -v, --verbose                    Display verbose output\n"
    "      --help                           Display this help and exit\n"
    "      --version                        Display version and exit\n"
    "      --debugseed                      Output seeds file for each reads (default: false)\n"
    "      --debugextend                    Show extension information (default: false)\n"
    "      --onlyseed                       Only search seeds file for each reads (default: false)\n"
    "      --nodp                           Don't use dp (default: false)\n"
    "      --split                          Split the uncorrected reads (default: false)\n"
    "      --devices=LIST                   HIP devices to use, e.g. 0,1,2,3 (default: 0)\n"
    "      --workers-per-device=N           batches in flight per device (default: 2; two are ~13 % faster than one)\n"
    "      --batch=N                        Reads per device batch (default: 100000)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace opt {
static int thread = 1;
static std::string prefix, directory, barcode, readsFile, saveIndex, mergeIndex;
static size_t PBcoverage = 90;
static double ErrorRate = 0.15;
static int startKmerLen = 19, nextTarget = 1, maxLeaves = 32, idmerLen = 9, minKmerLen = 13, genome = 10, mode = 1, verbose = 0;
static bool Split = false, DebugExtend = false, DebugSeed = false, OnlySeed = false, NoDp = false, Manual = false, Adjust = false;
static std::array<int, 3> offset = {{0, 0, 0}};
static std::vector<int> devices(1, 0);
static int workersPerDevice = 2;
static size_t batch = 100000;
static bool buildIndex = false, loadOnDevice = false;
}

static const char* shortopts = "t:p:o:b:c:e:k:u:r:n:l:i:s:g:m:v";
enum { OPT_HELP = 1, OPT_VERSION, OPT_SPLIT, OPT_FIRST, OPT_DEBUGEXTEND, OPT_DEBUGSEED, OPT_ONLYSEED, OPT_NODP, OPT_DEVICES, OPT_BATCH, OPT_WORKERS, OPT_BUILDINDEX, OPT_SAVEINDEX, OPT_LOADONDEVICE, OPT_MERGEINDEX };
static const struct option longopts[] = {
    {"thread", required_argument, nullptr, 't'},       {"prefix", required_argument, nullptr, 'p'},
    {"output", required_argument, nullptr, 'o'},       {"barcode", required_argument, nullptr, 'b'},
    {"PBcoverage", required_argument, nullptr, 'c'},   {"error-rate", required_argument, nullptr, 'e'},
    {"kmer-size", required_argument, nullptr, 'k'},    {"unique-offset", required_argument, nullptr, 'u'},
    {"repeat-offset", required_argument, nullptr, 'r'}, {"next-target", required_argument, nullptr, 'n'},
    {"max-leaves", required_argument, nullptr, 'l'},   {"idmer-length", required_argument, nullptr, 'i'},
    {"min-kmer-size", required_argument, nullptr, 's'}, {"genome", required_argument, nullptr, 'g'},
    {"mode", required_argument, nullptr, 'm'},         {"verbose", no_argument, nullptr, 'v'},
    {"help", no_argument, nullptr, OPT_HELP},          {"version", no_argument, nullptr, OPT_VERSION},
    {"split", no_argument, nullptr, OPT_SPLIT},        {"debugextend", no_argument, nullptr, OPT_DEBUGEXTEND},
    {"debugseed", no_argument, nullptr, OPT_DEBUGSEED}, {"onlyseed", no_argument, nullptr, OPT_ONLYSEED},
    {"nodp", no_argument, nullptr, OPT_NODP},          {"devices", required_argument, nullptr, OPT_DEVICES},
    {"batch", required_argument, nullptr, OPT_BATCH},  {"workers-per-device", required_argument, nullptr, OPT_WORKERS},
    {"build-index", no_argument, nullptr, OPT_BUILDINDEX}, {"save-index", required_argument, nullptr, OPT_SAVEINDEX},
    {"load-on-device", no_argument, nullptr, OPT_LOADONDEVICE}, {"merge-index", required_argument, nullptr, OPT_MERGEINDEX},
    {nullptr, 0, nullptr, 0}};

static void lrscOrDie(int st, const char* what)
{
    if(st != LRSC_OK) {
        std::cerr << what << ": " << lrsc_strerror(st) << " (" << lrsc_last_error() << ")\n";
        exit(EXIT_FAILURE);
    }
}

static void parsePacBioSelfCorrectionOptions(int argc, char** argv)
{
    optind = 1;
    bool die = false;
    for(int c; (c = getopt_long(argc, argv, shortopts, longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 't': arg >> opt::thread; break;
            case 'p': arg >> opt::prefix; break;
            case 'o': arg >> opt::directory; break;
            case 'b': arg >> opt::barcode; break;
            case 'c': arg >> opt::PBcoverage; break;
            case 'e': arg >> opt::ErrorRate; break;
            case 'k': arg >> opt::startKmerLen; opt::Adjust = true; break;
            case 'u': arg >> opt::offset[1]; opt::Adjust = true; break;
            case 'r': arg >> opt::offset[2]; opt::Adjust = true; break;
            case 'n': arg >> opt::nextTarget; break;
            case 'l': arg >> opt::maxLeaves; break;
            case 'i': arg >> opt::idmerLen; break;
            case 's': arg >> opt::minKmerLen; break;
            case 'g': arg >> opt::genome; break;
            case 'm': arg >> opt::mode; opt::Manual = true; break;
            case 'v': opt::verbose++; break;
            case OPT_HELP: std::cerr << CORRECT_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            case OPT_VERSION: std::cerr << CORRECT_VERSION_MESSAGE; exit(EXIT_SUCCESS);
            case OPT_SPLIT: opt::Split = true; break;
            case OPT_DEBUGEXTEND: opt::DebugExtend = true; break;
            case OPT_DEBUGSEED: opt::DebugSeed = true; break;
            case OPT_NODP: opt::NoDp = true; break;
            case OPT_ONLYSEED: opt::DebugSeed = true; opt::OnlySeed = true; break;
            case OPT_DEVICES: {
                opt::devices.clear();
                std::string tok;
                while(std::getline(arg, tok, ',')) opt::devices.push_back(atoi(tok.c_str()));
                break;
            }
            case OPT_BATCH: arg >> opt::batch; break;
            case OPT_WORKERS: arg >> opt::workersPerDevice; break;
            case OPT_BUILDINDEX: opt::buildIndex = true; break;
            case OPT_SAVEINDEX: arg >> opt::saveIndex; break;
            case OPT_LOADONDEVICE: opt::loadOnDevice = true; break;
            case OPT_MERGEINDEX: arg >> opt::mergeIndex; break;
            default: die = true; break;
        }
    }
    if(argc - optind < 1) { std::cerr << SUBPROGRAM ": missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << SUBPROGRAM ": too many arguments\n"; die = true; }
    if(opt::thread <= 0) { std::cerr << SUBPROGRAM ": invalid number of threads: " << opt::thread << "\n"; die = true; }
    if(opt::buildIndex && !opt::prefix.empty()) { std::cerr << SUBPROGRAM << ": --build-index reads no index files: give either it or -p\n"; die = true; }
    if(!opt::saveIndex.empty() && !opt::buildIndex) { std::cerr << SUBPROGRAM << ": --save-index writes the index that --build-index builds: give both\n"; die = true; }
    if(opt::loadOnDevice && opt::buildIndex) { std::cerr << SUBPROGRAM << ": --load-on-device decodes the index files that -p names: --build-index reads none\n"; die = true; }
    if(!opt::mergeIndex.empty() && !opt::buildIndex) { std::cerr << SUBPROGRAM << ": --merge-index merges PREFIX with the index that --build-index builds: give both\n"; die = true; }
    if(opt::prefix.empty() && !opt::buildIndex) { std::cerr << SUBPROGRAM << ": no prefix\n"; die = true; }
    if(opt::directory.empty()) { std::cerr << SUBPROGRAM << ": no directory\n"; die = true; }
    else {
        opt::directory += "/";
        // reference :346-363: with --debugseed the per-read files go to extend/ and seed/ (+ seed/error/)
        std::vector<std::string> subdir(1, std::string(""));
        if(opt::DebugSeed) { subdir.clear(); subdir.push_back("extend/"); subdir.push_back("seed/error/"); }
        for(const std::string& sub : subdir)
            if(system(("mkdir -p " + opt::directory + sub).c_str()) != 0) {
                std::cerr << SUBPROGRAM << ": something wrong making directory: " << opt::directory << "\n";
                die = true;
            }
    }
    if(opt::PBcoverage <= 0) { std::cerr << SUBPROGRAM ": invalid number of coverage: " << opt::PBcoverage << ", must be greater than zero\n"; die = true; }
    if(opt::ErrorRate < 0 || opt::ErrorRate > 1) { std::cerr << SUBPROGRAM ":invalid error rate: " << opt::ErrorRate << ", must be 0 ~ 1\n"; die = true; }
    if(opt::startKmerLen <= 0) { std::cerr << SUBPROGRAM ": invalid start kmer length: " << opt::startKmerLen << ", must be greater than zero\n"; die = true; }
    if(opt::nextTarget <= 0) { std::cerr << SUBPROGRAM ": invalid number of next target: " << opt::nextTarget << ", must be greater than zero\n"; die = true; }
    if(opt::maxLeaves <= 0) { std::cerr << SUBPROGRAM ":invalid number of max leaves:" << opt::maxLeaves << ", must be greater than zero\n"; die = true; }
    if(opt::idmerLen <= 0) { std::cerr << SUBPROGRAM ":invalid kmer length to identify similar reads" << opt::idmerLen << ", must be greater than zero\n"; die = true; }
    if(opt::minKmerLen <= 0) { std::cerr << SUBPROGRAM ":invalid min kmer length:" << opt::minKmerLen << ", must be greater than zero\n"; die = true; }
    if(opt::genome != 5 && opt::genome != 10 && opt::genome != 100) { std::cerr << SUBPROGRAM ": invalid genome size: " << opt::genome << ", must be (5/10/100)[m]\n"; die = true; }
    if(opt::mode < 0 || opt::mode > 2) { std::cerr << SUBPROGRAM ": invalid mode: " << opt::mode << ", must be (0/1/2)\n"; die = true; }
    if(opt::OnlySeed && opt::barcode.empty()) { std::cerr << SUBPROGRAM ": no barcode\n"; die = true; }
    if(opt::devices.empty() || opt::batch == 0 || opt::workersPerDevice < 1 || opt::workersPerDevice > 8) { std::cerr << SUBPROGRAM ": invalid --devices / --batch / --workers-per-device\n"; die = true; }
    if(die) { std::cerr << "\n" << CORRECT_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    opt::readsFile = argv[optind++];
}

// every read of the file, concatenated: read i is bases[off[i], off[i + 1])
static void loadReads(const std::string& path, std::string& bases, std::vector<uint64_t>& off)
{
    SeqReader reader(path);
    SeqRecord r;
    off.assign(1, 0);
    while(reader.get(r)) { bases += r.seq; off.push_back(bases.size()); }
}

// .sai / .rsai: lexicographic rank -> read index (SampledSuffixArray::buildLexicoIndex + writeLexicoIndex,
// SuffixTools/SampledSuffixArray.cpp:158-190,248-258; text format of SAWriter.cpp:32-54), here by the host sort of LexicoOrder.h:
// the reads are in hand.  `pbcorrect` only needs the file to exist.
static std::vector<uint32_t> lexicoOrder(const std::string& bases, const std::vector<uint64_t>& off, bool rev)
{
    return stride::lexicoOrder(bases.data(), off.data(), (uint32_t)(off.size() - 1), rev);
}
static bool writeSai(const std::string& path, const std::vector<uint32_t>& order)
{
    const size_t n = order.size();
    std::ofstream sai(path.c_str());
    sai << 51914 << "\n" << n << "\n" << n << "\n";
    for(size_t i = 0; i < n; ++i) sai << order[i] << " 0\n";
    if(!sai) { std::cerr << "index: cannot write " << path << "\n"; return false; }
    return true;
}
static bool writeLexicoIndex(const std::string& path, const std::string& bases, const std::vector<uint64_t>& off, bool rev)
{
    return writeSai(path, lexicoOrder(bases, off, rev));
}
// a .sai / .rsai file as writeSai leaves it: the read of every '$' row, in row order
static bool readSai(const std::string& path, uint64_t n_reads, std::vector<uint32_t>& order)
{
    std::ifstream sai(path.c_str());
    uint64_t magic = 0, n = 0, n2 = 0;
    sai >> magic >> n >> n2;
    order.assign(sai && magic == 51914 && n == n2 && n == n_reads ? n : 0, 0);
    uint64_t zero = 0;
    for(uint32_t& id : order) sai >> id >> zero;
    if(!sai || order.size() != n_reads) { std::cerr << "merge: " << path << " is no lexicographic index of " << n_reads << " reads\n"; return false; }
    return true;
}
// The '$' rows' reads of one strand of a saved index that is resident on `device`: its .sai / .rsai file where there is one,
// read and checked as ever; else from the index itself (lrsc_index_lexico_order, the reference's buildLexicoIndex).
static bool loadOrder(lrsc_index* idx, int device, const std::string& path, int rev, uint64_t n_reads, std::vector<uint32_t>& order)
{
    if(std::ifstream(path.c_str()).good()) return readSai(path, n_reads, order);
    order.assign(n_reads, 0);
    lrscOrDie(lrsc_index_lexico_order(idx, rev ? LRSC_RBWT : LRSC_BWT, device, order.data(), nullptr), "lrsc_index_lexico_order");
    return true;
}
// the union's list from its inputs': row k is b's next entry, its read ids behind a's, where from_b[k] is set, else a's next
// (lrsc_index_merge's dollar_origin of that strand)
static std::vector<uint32_t> mergeSai(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const uint8_t* from_b)
{
    std::vector<uint32_t> out(a.size() + b.size());
    size_t ia = 0, ib = 0;
    for(size_t k = 0; k < out.size(); ++k) {
        if(from_b[k] ? ib >= b.size() : ia >= a.size()) { std::cerr << "merge: the '$' rows of the merged index do not add up\n"; exit(EXIT_FAILURE); }
        out[k] = from_b[k] ? (uint32_t)(b[ib++] + a.size()) : a[ia++];
    }
    return out;
}

static int PacBioSelfCorrectionMain(int argc, char** argv)
{
    parsePacBioSelfCorrectionOptions(argc, argv);
    // --debugextend is accepted and inert: in the reference its only consumer (the debugExtInfo FASTA dump) is commented out
    // (PacBioSelfCorrectionProcess.cpp:87-98).
    PacBioSelfCorrectionParameters ecParams;
    lrsc_index* idx = nullptr;
    if(opt::buildIndex) {
        std::cerr << "Building the index of " << opt::readsFile << " on device " << opt::devices[0] << "\n";
        std::string bases;
        std::vector<uint64_t> off;
        loadReads(opt::readsFile, bases, off);
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)(off.size() - 1), opt::devices[0], &idx), "lrsc_index_build");
        std::vector<uint32_t> order[2];
        if(!opt::saveIndex.empty())
            for(int rev = 0; rev < 2; ++rev) order[rev] = lexicoOrder(bases, off, rev != 0);
        if(!opt::mergeIndex.empty()) {
            // the index to correct against: PREFIX's reads, then the reads just indexed
            std::cerr << "Merging it with " << opt::mergeIndex + BWT_EXT << " and " << opt::mergeIndex + RBWT_EXT << "\n";
            lrsc_index *old = nullptr, *both = nullptr;
            lrscOrDie(lrsc_index_open_device((opt::mergeIndex + BWT_EXT).c_str(), (opt::mergeIndex + RBWT_EXT).c_str(), opt::devices[0], &old), "lrsc_index_open_device");
            lrsc_index_info io, in;
            lrscOrDie(lrsc_index_info_get(old, &io), "lrsc_index_info_get");
            lrscOrDie(lrsc_index_info_get(idx, &in), "lrsc_index_info_get");
            const uint64_t n_all = io.num_strings + in.num_strings;
            std::vector<uint8_t> origin(opt::saveIndex.empty() ? 0 : 2 * n_all);
            lrscOrDie(lrsc_index_merge(old, idx, opt::devices[0], &both, origin.empty() ? nullptr : origin.data()), "lrsc_index_merge");
            for(int rev = 0; rev < 2 && !opt::saveIndex.empty(); ++rev) {
                std::vector<uint32_t> had;
                if(!loadOrder(old, opt::devices[0], opt::mergeIndex + (rev ? ".rsai" : ".sai"), rev, io.num_strings, had)) exit(EXIT_FAILURE);
                order[rev] = mergeSai(had, order[rev], origin.data() + rev * n_all);
            }
            lrsc_index_close(old);
            lrsc_index_close(idx);
            idx = both;
        }
        if(!opt::saveIndex.empty()) {
            lrscOrDie(lrsc_index_write(idx, opt::devices[0], (opt::saveIndex + BWT_EXT).c_str(), (opt::saveIndex + RBWT_EXT).c_str()), "lrsc_index_write");
            for(int rev = 0; rev < 2; ++rev)
                if(!writeSai(opt::saveIndex + (rev ? ".rsai" : ".sai"), order[rev])) exit(EXIT_FAILURE);
        }
    } else {
        std::cerr << "Loading BWT: " << opt::prefix + BWT_EXT << "\n" << "Loading RBWT: " << opt::prefix + RBWT_EXT << "\n";
        if(opt::loadOnDevice)   // resident on the first device; the others get the host image below
            lrscOrDie(lrsc_index_open_device((opt::prefix + BWT_EXT).c_str(), (opt::prefix + RBWT_EXT).c_str(), opt::devices[0], &idx), "lrsc_index_open_device");
        else
            lrscOrDie(lrsc_index_open((opt::prefix + BWT_EXT).c_str(), (opt::prefix + RBWT_EXT).c_str(), &idx), "lrsc_index_open");
    }
    for(int d : opt::devices) lrscOrDie(lrsc_index_upload(idx, d), "lrsc_index_upload");

    lrsc_params p;
    lrscOrDie(lrsc_params_default(opt::genome, (int)opt::PBcoverage, &p), "lrsc_params_default");
    if(opt::Adjust) {                       // -k/-u/-r given: no automatic derivation (reference :195-200)
        p.start_kmer_len = opt::startKmerLen;
        p.offset[0] = opt::offset[0]; p.offset[1] = opt::offset[1]; p.offset[2] = opt::offset[2];
    }
    p.error_rate = opt::ErrorRate; p.next_target = opt::nextTarget; p.max_leaves = opt::maxLeaves;
    p.idmer_len = opt::idmerLen; p.min_kmer_len = opt::minKmerLen; p.mode = opt::mode; p.manual = opt::Manual ? 1 : 0;
    p.split = opt::Split ? 1 : 0; p.no_dp = opt::NoDp ? 1 : 0;

    // one framework worker (host thread + lrsc_ctx) per entry: every device is listed workersPerDevice times, device-major order
    std::vector<int> workers;
    for(int w = 0; w < opt::workersPerDevice; ++w) for(int d : opt::devices) workers.push_back(d);
    ecParams.index = idx; ecParams.devices = workers; ecParams.directory = opt::directory; ecParams.p = p;
    ecParams.threads = opt::thread;
    ecParams.DebugExtend = opt::DebugExtend; ecParams.DebugSeed = opt::DebugSeed; ecParams.OnlySeed = opt::OnlySeed;
    if(opt::OnlySeed) BCode::load(opt::barcode);                   // reference :191

    {   // <out>/threshold-table (KmerThreshold.cpp:31-41,65-72)
        float thr[3 * 52];
        lrscOrDie(lrsc_kmer_thresholds(p.pb_coverage, thr), "lrsc_kmer_thresholds");
        std::ofstream t((opt::directory + "threshold-table").c_str());
        t << "Coverage : " << p.pb_coverage << "\n" << "size\tlowcov\tunique\trepeat\n";
        for(int k = 15; k <= 50; ++k) t << k << "\t" << thr[k] << "\t" << thr[52 + k] << "\t" << thr[104 + k] << "\n";
    }

    std::cerr << "\nCorrecting PacBio reads for " << opt::readsFile << " using--\n"
              << "number of threads:\t" << opt::thread << "\n"
              << "PB reads coverage:\t" << opt::PBcoverage << "\n"
              << "num of next Targets:\t" << opt::nextTarget << "\n"
              << "large kmer size:\t" << p.start_kmer_len << "\n"
              << "small kmer size:\t" << opt::minKmerLen << "\n"
              << "max leaves:\t" << opt::maxLeaves << "\n"
              << "max depth:\t1.2~0.8* (length between two seeds +- 20)" << "\n"
              << "devices:\t" << opt::devices.size() << " x " << opt::workersPerDevice << " workers\n";

    SequenceProcessFramework::processSequences<SequenceWorkItem, PacBioSelfCorrectionResult, PacBioSelfCorrectionProcess,
                                               PacBioSelfCorrectionPostProcess, PacBioSelfCorrectionParameters>(
        opt::thread, opt::readsFile, ecParams, opt::batch);
    lrsc_index_close(idx);
    return 0;
}

// `stride index -p PREFIX READS`: multi-string BWT of the reads and of the reversed reads on the GPU
static int indexMain(int argc, char** argv)
{
    std::string prefix, reads;
    int device = 0;
    for(int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if((a == "-p" || a == "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if(a.rfind("--prefix=", 0) == 0) prefix = a.substr(9);
        else if((a == "-t" || a == "-a" || a == "-d") && i + 1 < argc) ++i;     // accepted for compatibility, unused
        else if(a.rfind("--device=", 0) == 0) device = atoi(a.c_str() + 9);
        else if(a == "--help") { std::cerr << "Usage: " PACKAGE_NAME " index [-p PREFIX] [--device=N] READSFILE\n"; return 0; }
        else if(!a.empty() && a[0] != '-') reads = a;
    }
    if(reads.empty()) { std::cerr << "index: missing arguments\n"; return EXIT_FAILURE; }
    if(prefix.empty()) { prefix = reads.substr(reads.find_last_of('/') + 1); prefix = prefix.substr(0, prefix.find_last_of('.')); }
    std::string bases;
    std::vector<uint64_t> off;
    loadReads(reads, bases, off);
    const uint32_t n = (uint32_t)(off.size() - 1);
    std::cout << "Building index for " << reads << " on the GPU\n";
    for(int rev = 0; rev < 2; ++rev) {
        uint8_t* units = nullptr; uint64_t nu = 0;
        lrscOrDie(lrsc_build_bwt(bases.data(), off.data(), n, rev, device, &units, &nu), "lrsc_build_bwt");
        lrscOrDie(lrsc_write_bwt_file((prefix + (rev ? RBWT_EXT : BWT_EXT)).c_str(), units, nu, n, bases.size() + n), "lrsc_write_bwt_file");
        lrsc_buffer_free(units);
        if(!writeLexicoIndex(prefix + (rev ? ".rsai" : ".sai"), bases, off, rev != 0)) return EXIT_FAILURE;
    }
    return 0;
}

// `stride merge -p OUT PREFIX_A PREFIX_B [PREFIX_C ...]`: the index of A's reads followed by B's (then C's ...), merged on the
// device from the saved indexes; what `stride index` writes for the concatenated read files
static const char* MERGE_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " merge -p OUT [--device=N] PREFIX_A PREFIX_B [PREFIX_C ...]\n"
    "Merge the FM-indexes PREFIX_A, PREFIX_B, ... (.bwt, .rbwt, .sai, .rsai) into the index OUT of all their reads, in that order\n"
    "(an input's .sai / .rsai may be missing: it is then taken from its .bwt / .rbwt)\n"
    "\n"
    "      -p, --prefix=OUT                 Write OUT.bwt, OUT.rbwt, OUT.sai and OUT.rsai\n"
    "      --device=N                       HIP device to merge on (default: 0)\n"
    "      --help                           Display this help and exit\n\n";

static int mergeMain(int argc, char** argv)
{
    std::string prefix;
    std::vector<std::string> inputs;
    int device = 0;
    for(int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if((a == "-p" || a == "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if(a.rfind("--prefix=", 0) == 0) prefix = a.substr(9);
        else if(a.rfind("--device=", 0) == 0) device = atoi(a.c_str() + 9);
        else if(a == "--help") { std::cerr << MERGE_USAGE_MESSAGE; return 0; }
        else if(!a.empty() && a[0] != '-') inputs.push_back(a);
        else { std::cerr << "merge: unrecognized option " << a << "\n\n" << MERGE_USAGE_MESSAGE; return EXIT_FAILURE; }
    }
    if(prefix.empty()) { std::cerr << "merge: no prefix for the merged index (-p)\n\n" << MERGE_USAGE_MESSAGE; return EXIT_FAILURE; }
    if(inputs.size() < 2) { std::cerr << "merge: at least two indexes to merge\n\n" << MERGE_USAGE_MESSAGE; return EXIT_FAILURE; }

    struct Part { lrsc_index* idx = nullptr; uint64_t n_reads = 0; std::vector<uint32_t> order[2]; };
    auto open = [&](const std::string& p) {
        Part part;
        lrscOrDie(lrsc_index_open_device((p + BWT_EXT).c_str(), (p + RBWT_EXT).c_str(), device, &part.idx), "lrsc_index_open_device");
        lrsc_index_info info;
        lrscOrDie(lrsc_index_info_get(part.idx, &info), "lrsc_index_info_get");
        part.n_reads = info.num_strings;
        for(int rev = 0; rev < 2; ++rev)
            if(!loadOrder(part.idx, device, p + (rev ? ".rsai" : ".sai"), rev, part.n_reads, part.order[rev])) exit(EXIT_FAILURE);
        return part;
    };
    std::cout << "Merging " << inputs.size() << " indexes on the GPU\n";
    Part cur = open(inputs[0]);
    for(size_t k = 1; k < inputs.size(); ++k) {                   // ((A + B) + C) ...
        Part next = open(inputs[k]), both;
        both.n_reads = cur.n_reads + next.n_reads;
        std::vector<uint8_t> origin(2 * both.n_reads);
        lrscOrDie(lrsc_index_merge(cur.idx, next.idx, device, &both.idx, origin.data()), "lrsc_index_merge");
        for(int rev = 0; rev < 2; ++rev) both.order[rev] = mergeSai(cur.order[rev], next.order[rev], origin.data() + rev * both.n_reads);
        lrsc_index_close(cur.idx);
        lrsc_index_close(next.idx);
        cur = std::move(both);
    }
    lrscOrDie(lrsc_index_write(cur.idx, device, (prefix + BWT_EXT).c_str(), (prefix + RBWT_EXT).c_str()), "lrsc_index_write");
    for(int rev = 0; rev < 2; ++rev)
        if(!writeSai(prefix + (rev ? ".rsai" : ".sai"), cur.order[rev])) return EXIT_FAILURE;
    lrsc_index_close(cur.idx);
    return 0;
}

// `stride sai -p PREFIX`: PREFIX.sai and PREFIX.rsai from PREFIX.bwt and PREFIX.rbwt alone, the reference's buildLexicoIndex +
// writeLexicoIndex (SuffixTools/SampledSuffixArray.cpp:158-190,248-258) on an index that already exists
static const char* SAI_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " sai -p PREFIX [--device=N]\n"
    "Write the lexicographic index PREFIX.sai and PREFIX.rsai of the FM-index PREFIX.bwt and PREFIX.rbwt\n"
    "\n"
    "      -p, --prefix=PREFIX              Read PREFIX.bwt and PREFIX.rbwt, write PREFIX.sai and PREFIX.rsai\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "      --help                           Display this help and exit\n\n";

static int saiMain(int argc, char** argv)
{
    std::string prefix;
    int device = 0;
    for(int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if((a == "-p" || a == "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if(a.rfind("--prefix=", 0) == 0) prefix = a.substr(9);
        else if(a.rfind("--device=", 0) == 0) device = atoi(a.c_str() + 9);
        else if(a == "--help") { std::cerr << SAI_USAGE_MESSAGE; return 0; }
        else if(!a.empty() && a[0] != '-') { std::cerr << "sai: too many arguments\n\n" << SAI_USAGE_MESSAGE; return EXIT_FAILURE; }
        else { std::cerr << "sai: unrecognized option " << a << "\n\n" << SAI_USAGE_MESSAGE; return EXIT_FAILURE; }
    }
    if(prefix.empty()) { std::cerr << "sai: no prefix of the index (-p)\n\n" << SAI_USAGE_MESSAGE; return EXIT_FAILURE; }
    lrsc_index* idx = nullptr;
    lrscOrDie(lrsc_index_open_device((prefix + BWT_EXT).c_str(), (prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    std::cout << "Building the lexicographic index of " << prefix << " on the GPU\n";
    for(int rev = 0; rev < 2; ++rev) {
        std::vector<uint32_t> order(info.num_strings);
        lrscOrDie(lrsc_index_lexico_order(idx, rev ? LRSC_RBWT : LRSC_BWT, device, order.data(), nullptr), "lrsc_index_lexico_order");
        if(!writeSai(prefix + (rev ? ".rsai" : ".sai"), order)) return EXIT_FAILURE;
    }
    lrsc_index_close(idx);
    return 0;
}

// `stride grep READSFILE < queries`: the reads that hold a substring, the reference's grep (StriDe/grep.cpp:56-138): per query
// the rows of its interval in the .bwt, each located to its read (SampledSuffixArray::calcSA) and printed with the query's first
// occurrence in yellow; then every distinct read once, in first-seen order
static const char* GREP_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " grep [-p PREFIX] [--device=N] [--sample-rate=R] READSFILE\n"
    "Print the reads of READSFILE that hold the substrings given on the standard input, separated by white space\n"
    "\n"
    "      -p, --prefix=PREFIX              Use the FM-index PREFIX.bwt and PREFIX.rbwt (default: READSFILE's name without its suffix)\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "      --sample-rate=R                  Keep the suffix array of every R-th row; 0: walk every row back to the start of its read\n"
    "                                       (default: 32)\n"
    "      --help                           Display this help and exit\n\n";

static int grepMain(int argc, char** argv)
{
    std::string prefix;
    std::vector<std::string> files;
    int device = 0;
    long rate = 32;
    for(int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if((a == "-p" || a == "--prefix") && i + 1 < argc) prefix = argv[++i];
        else if(a.rfind("--prefix=", 0) == 0) prefix = a.substr(9);
        else if(a.rfind("--device=", 0) == 0) device = atoi(a.c_str() + 9);
        else if(a.rfind("--sample-rate=", 0) == 0) {
            char* end = nullptr;
            rate = strtol(a.c_str() + 14, &end, 10);
            if(end == a.c_str() + 14 || *end != 0 || rate < 0 || rate > 0x7FFFFFFFl) { std::cerr << "grep: invalid sample rate " << a.substr(14) << "\n\n" << GREP_USAGE_MESSAGE; return EXIT_FAILURE; }
        }
        else if(a == "--help") { std::cerr << GREP_USAGE_MESSAGE; return 0; }
        else if(!a.empty() && a[0] != '-') files.push_back(a);
        else { std::cerr << "grep: unrecognized option " << a << "\n\n" << GREP_USAGE_MESSAGE; return EXIT_FAILURE; }
    }
    if(files.empty()) { std::cerr << "grep: missing arguments\n\n" << GREP_USAGE_MESSAGE; return EXIT_FAILURE; }
    if(files.size() > 1) { std::cerr << "grep: too many arguments\n\n" << GREP_USAGE_MESSAGE; return EXIT_FAILURE; }
    const std::string& reads = files[0];
    if(prefix.empty()) { prefix = reads.substr(reads.find_last_of('/') + 1); prefix = prefix.substr(0, prefix.find_last_of('.')); }

    std::vector<SeqRecord> table;                                 // the reference's ReadTable
    {
        SeqReader reader(reads);
        SeqRecord r;
        while(reader.get(r)) { r.qual.clear(); table.push_back(r); }
    }
    lrsc_index* idx = nullptr;
    lrsc_ctx* ctx = nullptr;
    lrscOrDie(lrsc_index_open_device((prefix + BWT_EXT).c_str(), (prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    if(info.num_strings != table.size()) { std::cerr << "grep: " << prefix << " is no index of the " << table.size() << " reads of " << reads << "\n"; return EXIT_FAILURE; }
    lrscOrDie(lrsc_index_locate_prepare(idx, device, (uint32_t)rate), "lrsc_index_locate_prepare");
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");

    // the queries; their intervals in the .bwt, one lrsc_find_kmers call per length (field rvc of the reverse complement's search)
    std::vector<std::string> queries;
    for(std::string q; std::cin >> q;) queries.push_back(q);
    std::vector<lrsc_interval> interval(queries.size(), lrsc_interval{0, -1});
    std::map<size_t, std::vector<size_t>> by_len;
    for(size_t i = 0; i < queries.size(); ++i)
        if(queries[i].find_first_not_of("ACGT") == std::string::npos) by_len[queries[i].size()].push_back(i);
    for(const auto& kv : by_len) {
        std::string kmers;
        for(size_t i : kv.second) {
            const std::string& q = queries[i];
            for(size_t t = q.size(); t-- > 0;) kmers += q[t] == 'A' ? 'T' : q[t] == 'C' ? 'G' : q[t] == 'G' ? 'C' : 'A';
        }
        std::vector<lrsc_biinterval> iv(kv.second.size());
        lrscOrDie(lrsc_find_kmers(ctx, kmers.data(), (uint32_t)kv.first, kv.second.size(), iv.data()), "lrsc_find_kmers");
        for(size_t j = 0; j < kv.second.size(); ++j) interval[kv.second[j]] = iv[j].rvc;
    }
    // every row of every interval, located in one call
    std::vector<uint64_t> rows;
    for(const lrsc_interval& iv : interval)
        for(int64_t r = iv.lower; r <= iv.upper; ++r) rows.push_back((uint64_t)r);
    std::vector<lrsc_sa_elem> sa(rows.size());
    lrscOrDie(lrsc_locate(ctx, LRSC_BWT, rows.data(), rows.size(), sa.data()), "lrsc_locate");

    const char *yellow = "\033[33m", *plain = "\033[0m";
    std::vector<uint32_t> seen_order;
    std::vector<uint8_t> seen(table.size(), 0);
    size_t at = 0;
    for(size_t i = 0; i < queries.size(); ++i) {
        const std::string& q = queries[i];
        std::cout << "--\n";
        for(int64_t r = interval[i].lower; r <= interval[i].upper; ++r, ++at) {
            const uint32_t id = sa[at].read;
            const size_t found = id < table.size() ? table[id].seq.find(q) : std::string::npos;
            if(found == std::string::npos) { std::cerr << "grep: " << prefix << " is no index of the reads of " << reads << "\n"; return EXIT_FAILURE; }
            const std::string& read = table[id].seq;
            if(!seen[id]) { seen[id] = 1; seen_order.push_back(id); }
            std::cout << table[id].id << "\n" << read.substr(0, found) << yellow << read.substr(found, q.size()) << plain << read.substr(found + q.size()) << "\n";
        }
        std::cout << "--\n";
    }
    for(uint32_t id : seen_order) std::cout << ">" << table[id].id << "\n" << table[id].seq << "\n";
    std::cout.flush();
    lrsc_ctx_destroy(ctx);
    lrsc_index_close(idx);
    return 0;
}

// `stride filter READSFILE`: the reference's filter (StriDe/filter.cpp:48-70,120-319): every read is looked up in the index as a
// whole string; exact duplicates, reverse-complement duplicates and reads contained in another read go to the discard file, the
// others to the pass file, and the index of the passing reads is written beside them.  That index is the input's with the
// discarded reads taken out on the device (lrsc_index_remove), where the reference runs its index construction a second time.
static const char* FILTER_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " filter [OPTION] ... READSFILE\n"
    "Remove reads from a data set.\n"
    "The currently available filters are removing exact-match duplicates\n"
    "and removing reads with low-frequency k-mers.\n"
    "Automatically rebuilds the FM-index without the discarded reads.\n"
    "\n"
    "      --help                           display this help and exit\n"
    "      -v, --verbose                    display verbose output\n"
    "      -p, --prefix=PREFIX              use PREFIX for the names of the index files (default: prefix of the input file)\n"
    "      --build-index                    index READSFILE in memory on the device instead of loading PREFIX.bwt/.rbwt\n"
    "      -o, --outfile=FILE               write the qc-passed reads to FILE (default: READSFILE.filter.pass.fa)\n"
    "      -t, --threads=NUM                use NUM threads to compute the overlaps (default: 1)\n"
    "      -d, --sample-rate=N              use occurrence array sample rate of N in the FM-index. Higher values use significantly\n"
    "                                       less memory at the cost of higher runtime. This value must be a power of 2 (default: 128)\n"
    "      --no-duplicate-check             turn off duplicate removal\n"
    "      --substring-only                 when removing duplicates, only remove substring sequences, not full-length matches\n"
    "      --no-kmer-check                  turn off the kmer check\n"
    "      --homopolymer-check              check reads for hompolymer run length sequencing errors\n"
    "      --low-complexity-check           filter out low complexity reads\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "\nK-mer filter options:\n"
    "      -k, --kmer-size=N                The length of the kmer to use. (default: 31)\n"
    "      -x, --kmer-threshold=N           Require at least N kmer coverage for each kmer in a read. (default: 3)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace filteropt {
static unsigned int verbose = 0;
static int numThreads = 8, sampleRate = 128, kmerLength = 31, kmerThreshold = 3, device = 0;
static std::string prefix, readsFile, outFile, discardFile;
static bool dupCheck = true, substringOnly = false, hpCheck = false, lowComplexityCheck = false, buildIndex = false;
static const size_t batch = 100000;                             // reads per device call
}

// file name without its directory, a .gz suffix and its extension (Util/Util.cpp:218-225)
static std::string getFilename(const std::string& path)
{
    std::string out = path.substr(path.find_last_of('/') + 1);
    if(out.size() >= 3 && out.compare(out.size() - 3, 3, ".gz") == 0) out = out.substr(0, out.size() - 3);
    return out.substr(0, out.find_last_of('.'));
}

static void parseFilterOptions(int argc, char** argv)
{
    enum { F_HELP = 1, F_SUBSTRING_ONLY, F_NO_RMDUP, F_NO_KMER, F_CHECK_HPRUNS, F_CHECK_COMPLEXITY, F_DEVICE, F_BUILDINDEX };
    static const struct option filter_longopts[] = {
        {"verbose", no_argument, nullptr, 'v'},               {"threads", required_argument, nullptr, 't'},
        {"outfile", required_argument, nullptr, 'o'},         {"prefix", required_argument, nullptr, 'p'},
        {"sample-rate", required_argument, nullptr, 'd'},     {"kmer-size", required_argument, nullptr, 'k'},
        {"kmer-threshold", required_argument, nullptr, 'x'},  {"help", no_argument, nullptr, F_HELP},
        {"no-duplicate-check", no_argument, nullptr, F_NO_RMDUP}, {"no-kmer-check", no_argument, nullptr, F_NO_KMER},
        {"homopolymer-check", no_argument, nullptr, F_CHECK_HPRUNS}, {"low-complexity-check", no_argument, nullptr, F_CHECK_COMPLEXITY},
        {"substring-only", no_argument, nullptr, F_SUBSTRING_ONLY}, {"device", required_argument, nullptr, F_DEVICE},
        {"build-index", no_argument, nullptr, F_BUILDINDEX},  {nullptr, 0, nullptr, 0}};
    optind = 1;
    bool die = false;
    for(int c; (c = getopt_long(argc, argv, "p:d:t:o:k:x:v", filter_longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 'p': arg >> filteropt::prefix; break;
            case 'o': arg >> filteropt::outFile; break;
            case 't': arg >> filteropt::numThreads; break;
            case 'd': arg >> filteropt::sampleRate; break;
            case 'k': arg >> filteropt::kmerLength; break;
            case 'x': arg >> filteropt::kmerThreshold; break;
            case 'v': filteropt::verbose++; break;
            case F_NO_RMDUP: filteropt::dupCheck = false; break;
            case F_NO_KMER: break;                              // the k-mer check starts switched off and nothing switches it on
            case F_CHECK_HPRUNS: filteropt::hpCheck = true; break;
            case F_CHECK_COMPLEXITY: filteropt::lowComplexityCheck = true; break;
            case F_SUBSTRING_ONLY: filteropt::substringOnly = true; break;
            case F_DEVICE: arg >> filteropt::device; break;
            case F_BUILDINDEX: filteropt::buildIndex = true; break;
            case F_HELP: std::cout << FILTER_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            default: die = true; break;
        }
    }
    if(argc - optind < 1) { std::cerr << "filter: missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << "filter: too many arguments\n"; die = true; }
    if(filteropt::numThreads <= 0) { std::cerr << "filter: invalid number of threads: " << filteropt::numThreads << "\n"; die = true; }
    if(filteropt::kmerLength <= 0) { std::cerr << "filter: invalid kmer length: " << filteropt::kmerLength << ", must be greater than zero\n"; die = true; }
    if(filteropt::kmerThreshold <= 0) { std::cerr << "filter: invalid kmer threshold: " << filteropt::kmerThreshold << ", must be greater than zero\n"; die = true; }
    if(die) { std::cout << "\n" << FILTER_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    filteropt::readsFile = argv[optind++];
    if(filteropt::prefix.empty()) filteropt::prefix = getFilename(filteropt::readsFile);
    if(filteropt::outFile.empty()) {
        filteropt::outFile = filteropt::prefix + ".filter.pass.fa";
        filteropt::discardFile = filteropt::prefix + ".discard.fa";
    } else
        filteropt::discardFile = getFilename(filteropt::outFile) + ".discard.fa";
}

static int filterMain(int argc, char** argv)
{
    parseFilterOptions(argc, argv);
    const int device = filteropt::device;
    lrsc_index* idx = nullptr;
    if(filteropt::buildIndex) {
        std::string bases;
        std::vector<uint64_t> off;
        loadReads(filteropt::readsFile, bases, off);
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)(off.size() - 1), device, &idx), "lrsc_index_build");
    } else
        lrscOrDie(lrsc_index_open_device((filteropt::prefix + BWT_EXT).c_str(), (filteropt::prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    lrsc_ctx* ctx = nullptr;
    lrsc_dupcheck* session = nullptr;
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");
    lrscOrDie(lrsc_dupcheck_create(ctx, &session), "lrsc_dupcheck_create");

    QCParameters params;
    params.ctx = ctx;
    params.dupcheck = session;
    params.checkDuplicates = filteropt::dupCheck;
    params.substringOnly = filteropt::substringOnly;
    params.checkKmer = false;
    params.checkHPRuns = filteropt::hpCheck;
    params.checkDegenerate = filteropt::lowComplexityCheck;
    params.verbose = (int)filteropt::verbose;
    params.kmerLength = filteropt::kmerLength;
    params.kmerThreshold = filteropt::kmerThreshold;

    // the reads in file order, a batch per device call; drop[i] and the '$' interval of read i are kept for the index
    std::vector<uint8_t> drop;
    std::vector<lrsc_interval> own;
    {
        std::ofstream pass(filteropt::outFile.c_str()), discard(filteropt::discardFile.c_str());
        if(!pass || !discard) { std::cerr << "Error: could not open " << filteropt::outFile << " / " << filteropt::discardFile << " for write\n"; return EXIT_FAILURE; }
        QCProcess processor(params);
        QCPostProcess post(&pass, &discard);
        SeqReader reader(filteropt::readsFile);
        WorkItemGenerator<SequenceWorkItem> generator(&reader);
        std::vector<SequenceWorkItem> items;
        std::vector<lrsc_dup_result> dup;
        for(bool more = true; more;) {
            items.clear();
            SequenceWorkItem item;
            while(items.size() < filteropt::batch && (more = generator.generate(item))) items.push_back(item);
            const std::vector<QCResult> results = processor.process_batch(items, &dup);
            for(size_t i = 0; i < items.size(); ++i) {
                post.process(items[i], results[i]);
                drop.push_back(results[i].passed() ? 0 : 1);
                own.push_back(dup[i].fwd_dollar);
            }
        }
    }                                                             // the counters are printed here
    lrsc_dupcheck_destroy(session);
    lrsc_ctx_destroy(ctx);

    // Reads are taken out of the index by their number: the file has to be the index's read set.  Read i's own '$' row, the
    // inverse of the lexicographic order, must be one of the '$' rows of the reads equal to it.
    if(drop.size() != info.num_strings) {
        std::cerr << "filter: " << filteropt::readsFile << " holds " << drop.size() << " reads, the index " << filteropt::prefix << " " << info.num_strings
                  << ": no index written\n";
        return EXIT_FAILURE;
    }
    {
        std::vector<uint32_t> order(info.num_strings), row(info.num_strings);
        lrscOrDie(lrsc_index_lexico_order(idx, LRSC_BWT, device, order.data(), nullptr), "lrsc_index_lexico_order");
        for(size_t k = 0; k < order.size(); ++k) row[order[k]] = (uint32_t)k;
        for(size_t i = 0; i < row.size(); ++i)
            if((int64_t)row[i] < own[i].lower || (int64_t)row[i] > own[i].upper) {
                std::cerr << "filter: read " << i << " of " << filteropt::readsFile << " is not read " << i << " of the index " << filteropt::prefix
                          << " (the file is not the read set the index was made of): no index written\n";
                return EXIT_FAILURE;
            }
    }
    const std::string out_prefix = getFilename(filteropt::outFile);
    if(std::count(drop.begin(), drop.end(), 0) == 0) { std::cerr << "filter: no read passed: no index written\n"; return EXIT_FAILURE; }
    std::cout << "Making the index of " << filteropt::outFile << " from " << filteropt::prefix << " without the discarded reads on the GPU\n";
    lrsc_index* kept = nullptr;
    lrscOrDie(lrsc_index_remove(idx, drop.data(), drop.size(), device, &kept), "lrsc_index_remove");
    lrsc_index_close(idx);
    lrscOrDie(lrsc_index_write(kept, device, (out_prefix + BWT_EXT).c_str(), (out_prefix + RBWT_EXT).c_str()), "lrsc_index_write");
    lrsc_index_info kept_info;
    lrscOrDie(lrsc_index_info_get(kept, &kept_info), "lrsc_index_info_get");
    for(int rev = 0; rev < 2; ++rev) {
        std::vector<uint32_t> order(kept_info.num_strings);
        lrscOrDie(lrsc_index_lexico_order(kept, rev ? LRSC_RBWT : LRSC_BWT, device, order.data(), nullptr), "lrsc_index_lexico_order");
        if(!writeSai(out_prefix + (rev ? ".rsai" : ".sai"), order)) return EXIT_FAILURE;
    }
    lrsc_index_close(kept);
    return 0;
}

// `stride correct -a kmer READSFILE`: the reference's correct (StriDe/correct.cpp:44-78,145-258,312-465) with the k-mer algorithm
// (ErrorCorrectProcess::kmerCorrection) run on the device, a batch of reads per lrsc_kmer_correct call.  The overlap and hybrid
// algorithms are not built, and neither is --learn: it samples the index with rand() seeded from the clock.
static const char* KCORRECT_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " correct [OPTION] ... READSFILE\n"
    "Correct sequencing errors in all the reads in READSFILE\n"
    "\n"
    "      --help                           display this help and exit\n"
    "      -v, --verbose                    display verbose output\n"
    "      -p, --prefix=PREFIX              use PREFIX for the names of the index files (default: prefix of the input file)\n"
    "      --build-index                    index READSFILE in memory on the device instead of loading PREFIX.bwt/.rbwt\n"
    "      -o, --outfile=FILE               write the corrected reads to FILE (default: READSFILE.ec.fa)\n"
    "      -t, --threads=NUM                use NUM threads for the computation (default: 1)\n"
    "          --discard                    detect and discard low-quality reads\n"
    "      -d, --sample-rate=N              use occurrence array sample rate of N in the FM-index. Higher values use significantly\n"
    "                                       less memory at the cost of higher runtime. This value must be a power of 2 (default: 128)\n"
    "      -a, --algorithm=STR              specify the correction algorithm to use. STR must be one of kmer, hybrid, overlap. (default: kmer)\n"
    "          --metrics=FILE               collect error correction metrics (error rate by position in read, etc) and write them to FILE\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "\nKmer correction parameters:\n"
    "      -k, --kmer-size=N                The length of the kmer to use. (default: 31)\n"
    "      -x, --kmer-threshold=N           Attempt to correct kmers that are seen less than N times. (default: 3)\n"
    "      -i, --kmer-rounds=N              Perform N rounds of k-mer correction, correcting up to N bases (default: 10)\n"
    "          --learn                      Attempt to learn the k-mer correction threshold (experimental). Overrides -x parameter.\n"
    "\nOverlap correction parameters:\n"
    "      -e, --error-rate                 the maximum error rate allowed between two sequences to consider them overlapped (default: 0.04)\n"
    "      -m, --min-overlap=LEN            minimum overlap required between two reads (default: 45)\n"
    "      -c, --conflict=INT               use INT as the threshold to detect a conflicted base in the multi-overlap (default: 5)\n"
    "      -l, --seed-length=LEN            force the seed length to be LEN. By default, the seed length in the overlap step\n"
    "                                       is calculated to guarantee all overlaps with --error-rate differences are found.\n"
    "                                       This option removes the guarantee but will be (much) faster. As SGA can tolerate some\n"
    "                                       missing edges, this option may be preferable for some data sets.\n"
    "      -s, --seed-stride=LEN            force the seed stride to be LEN. This parameter will be ignored unless --seed-length\n"
    "                                       is specified (see above). This parameter defaults to the same value as --seed-length\n"
    "      -b, --branch-cutoff=N            stop the overlap search at N branches. This parameter is used to control the search time for\n"
    "                                       highly-repetitive reads. If the number of branches exceeds N, the search stops and the read\n"
    "                                       will not be corrected. This is not enabled by default.\n"
    "      -r, --rounds=NUM                 iteratively correct reads up to a maximum of NUM rounds (default: 1)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace correctopt {
static unsigned int verbose = 0;
static int numThreads = 1, numOverlapRounds = 1, sampleRate = 128, seedLength = 0, seedStride = 0, conflictCutoff = 3, branchCutoff = -1;
static int kmerLength = 31, kmerThreshold = 3, numKmerRounds = 10, device = 0;
static unsigned int minOverlap = 45;
static double errorRate = 0.04;
static std::string prefix, readsFile, outFile, discardFile, metricsFile;
static bool buildIndex = false;
static const size_t batch = 100000;                             // reads per device call
}

static void parseCorrectOptions(int argc, char** argv)
{
    enum { C_HELP = 1, C_VERSION, C_METRICS, C_DISCARD, C_LEARN, C_DIPLOID, C_DEVICE, C_BUILDINDEX };
    static const struct option correct_longopts[] = {
        {"verbose", no_argument, nullptr, 'v'},               {"threads", required_argument, nullptr, 't'},
        {"min-overlap", required_argument, nullptr, 'm'},     {"rounds", required_argument, nullptr, 'r'},
        {"outfile", required_argument, nullptr, 'o'},         {"prefix", required_argument, nullptr, 'p'},
        {"error-rate", required_argument, nullptr, 'e'},      {"seed-length", required_argument, nullptr, 'l'},
        {"seed-stride", required_argument, nullptr, 's'},     {"algorithm", required_argument, nullptr, 'a'},
        {"sample-rate", required_argument, nullptr, 'd'},     {"conflict", required_argument, nullptr, 'c'},
        {"branch-cutoff", required_argument, nullptr, 'b'},   {"kmer-size", required_argument, nullptr, 'k'},
        {"kmer-threshold", required_argument, nullptr, 'x'},  {"kmer-rounds", required_argument, nullptr, 'i'},
        {"learn", no_argument, nullptr, C_LEARN},             {"discard", no_argument, nullptr, C_DISCARD},
        {"help", no_argument, nullptr, C_HELP},               {"version", no_argument, nullptr, C_VERSION},
        {"metrics", required_argument, nullptr, C_METRICS},   {"diploid", no_argument, nullptr, C_DIPLOID},
        {"device", required_argument, nullptr, C_DEVICE},     {"build-index", no_argument, nullptr, C_BUILDINDEX},
        {nullptr, 0, nullptr, 0}};
    optind = 1;
    std::string algo_str;
    bool discardReads = false, learn = false, die = false;
    for(int c; (c = getopt_long(argc, argv, "p:m:d:e:t:l:s:o:r:b:a:c:k:x:i:v", correct_longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 'm': arg >> correctopt::minOverlap; break;
            case 'p': arg >> correctopt::prefix; break;
            case 'o': arg >> correctopt::outFile; break;
            case 'e': arg >> correctopt::errorRate; break;
            case 't': arg >> correctopt::numThreads; break;
            case 'l': arg >> correctopt::seedLength; break;
            case 's': arg >> correctopt::seedStride; break;
            case 'r': arg >> correctopt::numOverlapRounds; break;
            case 'a': arg >> algo_str; break;
            case 'd': arg >> correctopt::sampleRate; break;
            case 'c': arg >> correctopt::conflictCutoff; break;
            case 'k': arg >> correctopt::kmerLength; break;
            case 'x': arg >> correctopt::kmerThreshold; break;
            case 'v': correctopt::verbose++; break;
            case 'b': arg >> correctopt::branchCutoff; break;
            case 'i': arg >> correctopt::numKmerRounds; break;
            case C_LEARN: learn = true; break;
            case C_DISCARD: discardReads = true; break;
            case C_METRICS: arg >> correctopt::metricsFile; break;
            case C_DIPLOID: break;                                // read by the overlap algorithm only
            case C_DEVICE: arg >> correctopt::device; break;
            case C_BUILDINDEX: correctopt::buildIndex = true; break;
            case C_HELP: std::cout << KCORRECT_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            case C_VERSION: std::cout << "correct Version " PACKAGE_VERSION " (MI355X back end)\n"; exit(EXIT_SUCCESS);
            default: die = true; break;
        }
    }
    if(argc - optind < 1) { std::cerr << "correct: missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << "correct: too many arguments\n"; die = true; }
    if(correctopt::numThreads <= 0) { std::cerr << "correct: invalid number of threads: " << correctopt::numThreads << "\n"; die = true; }
    if(correctopt::numOverlapRounds <= 0) { std::cerr << "correct: invalid number of overlap rounds: " << correctopt::numOverlapRounds << ", must be at least 1\n"; die = true; }
    if(correctopt::numKmerRounds <= 0) { std::cerr << "correct: invalid number of kmer rounds: " << correctopt::numKmerRounds << ", must be at least 1\n"; die = true; }
    if(correctopt::kmerLength <= 0) { std::cerr << "correct: invalid kmer length: " << correctopt::kmerLength << ", must be greater than zero\n"; die = true; }
    if(correctopt::kmerThreshold <= 0) { std::cerr << "correct: invalid kmer threshold: " << correctopt::kmerThreshold << ", must be greater than zero\n"; die = true; }
    if(algo_str.empty()) {
        // the reference starts from the overlap algorithm, whatever its usage text says of the default
        std::cerr << "correct: without -a the reference runs its overlap algorithm, which is not built here: say -a kmer\n";
        die = true;
    } else if(algo_str == "hybrid" || algo_str == "overlap") {
        std::cerr << "correct: -a " << algo_str << " is not built here: only -a kmer is\n";
        die = true;
    } else if(algo_str != "kmer") {
        std::cerr << "correct: unrecognized -a,--algorithm parameter: " << algo_str << "\n";
        die = true;
    }
    if(learn) { std::cerr << "correct: --learn is not built here (it samples the index at random, seeded from the clock): set -x\n"; die = true; }
    if(die) { std::cout << "\n" << KCORRECT_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    if(correctopt::errorRate > 1.0f) { std::cerr << "Invalid error-rate parameter: " << correctopt::errorRate << "\n"; exit(EXIT_FAILURE); }
    correctopt::readsFile = argv[optind++];
    if(correctopt::prefix.empty()) correctopt::prefix = getFilename(correctopt::readsFile);
    const std::string out_prefix = getFilename(correctopt::readsFile);
    if(correctopt::outFile.empty()) correctopt::outFile = out_prefix + ".ec.fa";
    correctopt::discardFile = discardReads ? out_prefix + ".discard.fa" : std::string();
}

static int correctMain(int argc, char** argv)
{
    parseCorrectOptions(argc, argv);
    const int device = correctopt::device;
    std::cout << "Correcting sequencing errors for " << correctopt::readsFile << "\n";
    lrsc_index* idx = nullptr;
    if(correctopt::buildIndex) {
        std::string bases;
        std::vector<uint64_t> off;
        loadReads(correctopt::readsFile, bases, off);
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)(off.size() - 1), device, &idx), "lrsc_index_build");
    } else {
        std::cout << "Loading BWT: " << correctopt::prefix + BWT_EXT << " and " << correctopt::prefix + RBWT_EXT << std::endl;
        lrscOrDie(lrsc_index_open_device((correctopt::prefix + BWT_EXT).c_str(), (correctopt::prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    }
    lrsc_ctx* ctx = nullptr;
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");

    ErrorCorrectParameters params;
    params.ctx = ctx;
    params.kmerLength = correctopt::kmerLength;
    params.kmerThreshold = correctopt::kmerThreshold;
    params.numKmerRounds = correctopt::numKmerRounds;
    params.readsFile = correctopt::readsFile;
    std::cout << "Perform error correction using" << std::endl
              << "kmer size=" << params.kmerLength << std::endl
              << "kmer threshold=" << correctopt::kmerThreshold << std::endl
              << "overlap rounds=" << correctopt::numOverlapRounds << std::endl;
    {
        std::ofstream writer(correctopt::outFile.c_str()), discard;
        if(!correctopt::discardFile.empty()) discard.open(correctopt::discardFile.c_str());
        if(!writer || (!correctopt::discardFile.empty() && !discard)) {
            std::cerr << "Error: could not open " << correctopt::outFile << (correctopt::discardFile.empty() ? "" : " / " + correctopt::discardFile) << " for write\n";
            return EXIT_FAILURE;
        }
        const bool collectMetrics = !correctopt::metricsFile.empty();
        ErrorCorrectProcess processor(params);
        ErrorCorrectPostProcess post(&writer, correctopt::discardFile.empty() ? nullptr : &discard, collectMetrics);
        SeqReader reader(correctopt::readsFile, true);
        WorkItemGenerator<SequenceWorkItem> generator(&reader);
        std::vector<SequenceWorkItem> items;
        for(bool more = true; more;) {
            items.clear();
            SequenceWorkItem item;
            while(items.size() < correctopt::batch && (more = generator.generate(item))) items.push_back(item);
            const std::vector<ErrorCorrectResult> results = processor.process_batch(items);
            for(size_t i = 0; i < items.size(); ++i) post.process(items[i], results[i]);
        }
        if(collectMetrics) {
            std::ofstream metrics(correctopt::metricsFile.c_str());
            if(!metrics) { std::cerr << "Error: could not open " << correctopt::metricsFile << " for write\n"; return EXIT_FAILURE; }
            post.writeMetrics(&metrics);
        }
    }                                                             // the counters are printed here
    std::cout.flush();
    lrsc_ctx_destroy(ctx);
    lrsc_index_close(idx);
    return 0;
}

// `stride fmwalk -a merge READSFILE`: the reference's FMIndexWalk (StriDe/FMIndexWalk.cpp:40-58,112-238,244-362) with the merge
// algorithm (FMIndexWalkProcess::MergePairedReads) run on the device, a batch of pairs per lrsc_fmwalk_merge call.  Not taken over
// in merge mode: the empty kmerized.fa that the reference opens and never writes, and the `Median kmer frequency` line, which comes
// from 100000 rand() samples that merge mode does not use.
// `stride fmwalk --hybrid PAIRS` and `--kmerize READS` run the reference's hybrid (MergeAndKmerize) and kmerize (KmerizeReads)
// algorithms the same way, lrsc_fmwalk_hybrid and lrsc_fmwalk_kmerize per batch; hybrid draws its 100000 sample rows as the
// reference does (rand() % the index's strings, unseeded) and takes their counts from lrsc_kmer_sample_counts.  `-a hybrid`, `-a
// kmerize` and an omitted -a are still refused: the two long options are how these modes are reached.
// `stride fmwalk --validate READS` runs the validate algorithm (ValidateReads), lrsc_fmwalk_validate per batch of single reads: the
// merged reads go to PREFIX.origin.fa (-o), the kmerized ones to PREFIX.kmerized.fa, and the reads that are neither to
// LowComplexityReads.fa in the working directory, as in the reference (FMIndexWalkProcess.cpp:908-909).  `-a validate` is still
// refused, like the other two.
static const char* FMWALK_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " FMIndexWalk [OPTION] ... READSFILE\n"
    "Merge paired end reads into long reads via FM-index walk\n"
    "\n"
    "      --help                           display this help and exit\n"
    "      -v, --verbose                    display verbose output\n"
    "      -p, --prefix=PREFIX              use PREFIX for the names of the index files (default: prefix of the input file)\n"
    "      --build-index                    index READSFILE in memory on the device instead of loading PREFIX.bwt/.rbwt\n"
    "      --load-on-device                 decode PREFIX.bwt/.rbwt on the device (what loading does here; accepted for symmetry)\n"
    "      -o, --outfile=FILE               write the corrected reads to FILE (default: READSFILE.ec.fa)\n"
    "      -t, --threads=NUM                use NUM threads for the computation (default: 1)\n"
    "      -a, --algorithm=STR              specify the walking algorithm (hybrid (default), merge, kmerize, or validate)\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "      --hybrid                         READSFILE holds pairs: merge them or cut them at unreliable kmers (no -a; --repeat-cutoff=N skips the sampling)\n"
    "      --kmerize                        READSFILE holds single reads: cut them at unreliable kmers (no -a)\n"
    "      --validate                       READSFILE holds single reads: validate each by walks from end to end, else cut it (no -a)\n"
    "\nAlgorithm parameters:\n"
    "      -k, --kmer-size=N                The length of the kmer to use. (default: 31)\n"
    "      -x, --kmer-threshold=N           Attempt to correct kmers that are seen less than N times. (default: 3)\n"
    "      -L, --max-leaves=N               Number of maximum leaves in the search tree (default: 32)\n"
    "      -I, --max-insertsize=N           the maximum insert size (i.e. search depth) (deault: 400)\n"
    "      -m, --min-overlap=N           the min overlap (default: 81)\n"
    "      -M, --max-overlap=N           the max overlap (default: avg read length*0.9)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace fmwalkopt {
static unsigned int verbose = 0;
static int numThreads = 1, kmerLength = 31, kmerThreshold = 3, maxLeaves = 32, maxInsertSize = 400, minOverlap = 81, maxOverlap = -1, device = 0;
static std::string prefix, readsFile, outFile, discardFile;
static bool buildIndex = false, hybrid = false, kmerize = false, validate = false;
static const char* const lowComplexFile = "LowComplexityReads.fa";    // FMIndexWalkProcess.cpp:908-909: in the working directory
static long long repeatCutoff = -1;                             // --repeat-cutoff: -1, from the sample
static const size_t batch = 100000;                             // pairs per device call
}

static void parseFMWalkOptions(int argc, char** argv)
{
    enum { F_HELP = 1, F_VERSION, F_METRICS, F_DISCARD, F_LEARN, F_DEVICE, F_BUILDINDEX, F_LOADONDEVICE, F_HYBRID, F_KMERIZE, F_REPEATCUTOFF, F_VALIDATE };
    static const struct option fmwalk_longopts[] = {
        {"verbose", no_argument, nullptr, 'v'},               {"threads", required_argument, nullptr, 't'},
        {"outfile", required_argument, nullptr, 'o'},         {"prefix", required_argument, nullptr, 'p'},
        {"algorithm", required_argument, nullptr, 'a'},       {"kmer-size", required_argument, nullptr, 'k'},
        {"kmer-threshold", required_argument, nullptr, 'x'},  {"max-leaves", required_argument, nullptr, 'L'},
        {"max-insertsize", required_argument, nullptr, 'I'},  {"min-overlap", required_argument, nullptr, 'm'},
        {"max-overlap", required_argument, nullptr, 'M'},     // the reference's table lacks it, its usage text names it
        {"learn", no_argument, nullptr, F_LEARN},             {"discard", no_argument, nullptr, F_DISCARD},
        {"help", no_argument, nullptr, F_HELP},               {"version", no_argument, nullptr, F_VERSION},
        {"metrics", required_argument, nullptr, F_METRICS},   {"device", required_argument, nullptr, F_DEVICE},
        {"build-index", no_argument, nullptr, F_BUILDINDEX},  {"load-on-device", no_argument, nullptr, F_LOADONDEVICE},
        {"hybrid", no_argument, nullptr, F_HYBRID},           {"kmerize", no_argument, nullptr, F_KMERIZE},
        {"repeat-cutoff", required_argument, nullptr, F_REPEATCUTOFF},
        {"validate", no_argument, nullptr, F_VALIDATE},
        {nullptr, 0, nullptr, 0}};
    optind = 1;
    std::string algo_str;
    bool die = false;
    for(int c; (c = getopt_long(argc, argv, "p:t:o:a:k:x:L:I:m:M:v", fmwalk_longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 'p': arg >> fmwalkopt::prefix; break;
            case 'o': arg >> fmwalkopt::outFile; break;
            case 't': arg >> fmwalkopt::numThreads; break;
            case 'a': arg >> algo_str; break;
            case 'k': arg >> fmwalkopt::kmerLength; break;
            case 'x': arg >> fmwalkopt::kmerThreshold; break;
            case 'v': fmwalkopt::verbose++; break;
            case 'L': arg >> fmwalkopt::maxLeaves; break;
            case 'I': arg >> fmwalkopt::maxInsertSize; break;
            case 'm': arg >> fmwalkopt::minOverlap; break;
            case 'M': arg >> fmwalkopt::maxOverlap; break;
            case F_LEARN: case F_DISCARD: case F_METRICS: case F_LOADONDEVICE: break;     // read and not used, as in the reference
            case F_DEVICE: arg >> fmwalkopt::device; break;
            case F_BUILDINDEX: fmwalkopt::buildIndex = true; break;
            case F_HYBRID: fmwalkopt::hybrid = true; break;
            case F_KMERIZE: fmwalkopt::kmerize = true; break;
            case F_VALIDATE: fmwalkopt::validate = true; break;
            case F_REPEATCUTOFF: arg >> fmwalkopt::repeatCutoff; break;
            case F_HELP: std::cout << FMWALK_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            case F_VERSION: std::cout << "FMIndexWalk Version " PACKAGE_VERSION " (MI355X back end)\n"; exit(EXIT_SUCCESS);
            default: die = true; break;
        }
    }
    if(argc - optind < 1) { std::cerr << "FMIndexWalk: missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << "FMIndexWalk: too many arguments\n"; die = true; }
    if(fmwalkopt::numThreads <= 0) { std::cerr << "FMIndexWalk: invalid number of threads: " << fmwalkopt::numThreads << "\n"; die = true; }
    if(fmwalkopt::kmerLength <= 0) { std::cerr << "FMIndexWalk: invalid kmer length: " << fmwalkopt::kmerLength << ", must be greater than zero\n"; die = true; }
    if(fmwalkopt::kmerThreshold <= 0) { std::cerr << "FMIndexWalk: invalid kmer threshold: " << fmwalkopt::kmerThreshold << ", must be greater than zero\n"; die = true; }
    if(fmwalkopt::validate) {
        if(fmwalkopt::hybrid || fmwalkopt::kmerize) {
            std::cerr << "FMIndexWalk: --validate and " << (fmwalkopt::hybrid ? "--hybrid" : "--kmerize") << " are two algorithms: give one\n";
            die = true;
        } else if(!algo_str.empty()) {
            std::cerr << "FMIndexWalk: -a is not given together with --validate\n";
            die = true;
        } else if(fmwalkopt::minOverlap < 2) {
            std::cerr << "FMIndexWalk: invalid min overlap: " << fmwalkopt::minOverlap << "\n";
            die = true;
        }
    } else if(fmwalkopt::hybrid || fmwalkopt::kmerize) {
        if(fmwalkopt::hybrid && fmwalkopt::kmerize) { std::cerr << "FMIndexWalk: --hybrid and --kmerize are two algorithms: give one\n"; die = true; }
        else if(!algo_str.empty()) {
            std::cerr << "FMIndexWalk: -a is not given together with " << (fmwalkopt::hybrid ? "--hybrid" : "--kmerize") << "\n";
            die = true;
        }
        if(fmwalkopt::repeatCutoff < -1) { std::cerr << "FMIndexWalk: invalid repeat cutoff: " << fmwalkopt::repeatCutoff << "\n"; die = true; }
    } else if(algo_str.empty()) {
        std::cerr << "FMIndexWalk: without -a the reference runs its hybrid algorithm, which is not built here: say -a merge\n";
        die = true;
    } else if(algo_str == "hybrid" || algo_str == "kmerize" || algo_str == "validate") {
        std::cerr << "FMIndexWalk: -a " << algo_str << " is not built here: only -a merge is\n";
        die = true;
    } else if(algo_str != "merge") {
        std::cerr << "FMIndexWalk: unrecognized -a,--algorithm parameter: " << algo_str << "\n";
        die = true;
    }
    if(die) { std::cout << "\n" << FMWALK_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    fmwalkopt::readsFile = argv[optind++];
    if(fmwalkopt::prefix.empty()) fmwalkopt::prefix = getFilename(fmwalkopt::readsFile);
    // StriDe/FMIndexWalk.cpp:346-361
    if(fmwalkopt::outFile.empty()) fmwalkopt::outFile = getFilename(fmwalkopt::readsFile) + (fmwalkopt::kmerize || fmwalkopt::validate ? ".origin.fa" : ".merge.fa");
    if(fmwalkopt::hybrid || fmwalkopt::kmerize || fmwalkopt::validate) fmwalkopt::discardFile = getFilename(fmwalkopt::readsFile) + ".kmerized.fa";
}

// StriDe/FMIndexWalk.cpp:147-154: the 100000 sampled counts of min-overlap-mers from .rbwt, the line about them, and
// isSuitableForFMWalk's cutoff.  rand() is the reference's: unseeded, % the index's strings.
static size_t fmwalkRepeatCutoff(lrsc_index* idx, lrsc_ctx* ctx)
{
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    const uint32_t samples = 100000;
    std::vector<uint64_t> rows(samples);
    for(uint32_t i = 0; i < samples; ++i) rows[i] = (uint64_t)rand() % info.num_strings;
    std::vector<uint32_t> counts(samples);
    lrscOrDie(lrsc_kmer_sample_counts(ctx, rows.data(), samples, (uint32_t)fmwalkopt::minOverlap, counts.data()), "lrsc_kmer_sample_counts");
    KmerDistribution kd;
    for(uint32_t i = 0; i < samples; ++i) kd.add((int)counts[i]);
    kd.computeKDAttributes();
    std::cout << "Median kmer frequency: " << kd.getQuartile(2) << "\t Std: " << kd.getSdv() << "\t 95% kmer frequency: " << kd.getCutoffForProportion(0.95)
              << "\t Repeat frequency cutoff: " << kd.getRepeatKmerCutoff() << "\n";
    return (size_t)(kd.getQuartile(2) * 1.3);
}

static int fmwalkMain(int argc, char** argv)
{
    parseFMWalkOptions(argc, argv);
    const int device = fmwalkopt::device;
    lrsc_index* idx = nullptr;
    if(fmwalkopt::buildIndex) {
        std::string bases;
        std::vector<uint64_t> off;
        loadReads(fmwalkopt::readsFile, bases, off);
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)(off.size() - 1), device, &idx), "lrsc_index_build");
    } else {
        std::cout << std::endl << "Loading BWT: " << fmwalkopt::prefix + BWT_EXT << "\n";
        std::cout << "Loading RBWT: " << fmwalkopt::prefix + RBWT_EXT << "\n";
        lrscOrDie(lrsc_index_open_device((fmwalkopt::prefix + BWT_EXT).c_str(), (fmwalkopt::prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    }
    lrsc_ctx* ctx = nullptr;
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");

    FMIndexWalkParameters params;
    params.ctx = ctx;
    params.kmerLength = fmwalkopt::kmerLength;
    params.kmerThreshold = fmwalkopt::kmerThreshold;
    params.maxLeaves = fmwalkopt::maxLeaves;
    params.maxInsertSize = fmwalkopt::maxInsertSize;
    params.minOverlap = fmwalkopt::minOverlap;
    params.maxOverlap = fmwalkopt::maxOverlap;
    params.algorithm = fmwalkopt::hybrid ? FMW_HYBRID : fmwalkopt::kmerize ? FMW_KMERIZE : fmwalkopt::validate ? FMW_VALIDATE : FMW_MERGE;
    if(fmwalkopt::hybrid) {
        if(fmwalkopt::minOverlap <= 0) { std::cerr << "FMIndexWalk: invalid min overlap: " << fmwalkopt::minOverlap << "\n"; return EXIT_FAILURE; }
        params.repeatKmerFreq = fmwalkopt::repeatCutoff >= 0 ? (size_t)fmwalkopt::repeatCutoff : fmwalkRepeatCutoff(idx, ctx);
    }
    bool odd = false;
    {
        std::ofstream writer(fmwalkopt::outFile.c_str());
        if(!writer) { std::cerr << "Error: could not open " << fmwalkopt::outFile << " for write\n"; return EXIT_FAILURE; }
        std::ofstream discard;
        if(!fmwalkopt::discardFile.empty()) {
            discard.open(fmwalkopt::discardFile.c_str());
            if(!discard) { std::cerr << "Error: could not open " << fmwalkopt::discardFile << " for write\n"; return EXIT_FAILURE; }
        }
        std::ofstream lowComplex;
        if(fmwalkopt::validate) {
            lowComplex.open(fmwalkopt::lowComplexFile);
            if(!lowComplex) { std::cerr << "Error: could not open " << fmwalkopt::lowComplexFile << " for write\n"; return EXIT_FAILURE; }
        }
        std::cout << "Merge paired end reads into long reads for " << fmwalkopt::readsFile << " using \n"
                  << "min overlap=" << params.minOverlap << "\t"
                  << "max overlap=" << params.maxOverlap << "\t"
                  << "max leaves=" << params.maxLeaves << "\t"
                  << "max Insert size=" << params.maxInsertSize << "\t"
                  << "kmer size=" << params.kmerLength << "\n\n";
        FMIndexWalkProcess processor(params);
        FMIndexWalkPostProcess post(&writer, fmwalkopt::discardFile.empty() ? nullptr : &discard, params.algorithm, fmwalkopt::validate ? &lowComplex : nullptr);
        SeqReader reader(fmwalkopt::readsFile, true);
        WorkItemGenerator<SequenceWorkItem> generator(&reader);
        const bool single = fmwalkopt::kmerize || fmwalkopt::validate;
        if(single) {
            std::vector<SequenceWorkItem> reads;
            for(bool more = true; more;) {
                reads.clear();
                SequenceWorkItem item;
                while(reads.size() < 2 * fmwalkopt::batch && (more = generator.generate(item))) reads.push_back(item);
                const std::vector<FMIndexWalkResult> results = processor.process_batch(reads);
                for(size_t i = 0; i < reads.size(); ++i) post.process(reads[i], results[i]);
            }
        }
        std::vector<SequenceWorkItemPair> pairs;
        for(bool more = !single; more;) {
            pairs.clear();
            SequenceWorkItemPair pair;
            while(pairs.size() < fmwalkopt::batch && (more = generator.generate(pair, &odd))) pairs.push_back(pair);
            if(odd) break;
            const std::vector<FMIndexWalkResult> results = processor.process_batch(pairs);
            for(size_t i = 0; i < pairs.size(); ++i) post.process(pairs[i], results[i]);
        }
    }                                                             // the counters are printed here
    std::cout.flush();
    lrsc_ctx_destroy(ctx);
    lrsc_index_close(idx);
    if(odd) {                                                     // the reference asserts
        std::cerr << "FMIndexWalk: " << fmwalkopt::readsFile << " holds an odd number of records: the reads of a pair follow one another\n";
        std::remove(fmwalkopt::outFile.c_str());
        if(!fmwalkopt::discardFile.empty()) std::remove(fmwalkopt::discardFile.c_str());
        return EXIT_FAILURE;
    }
    return 0;
}

// `stride overlap READSFILE`: the reference's overlap (StriDe/overlap.cpp:126-413) in its default mode, errorRate = -1: the exact
// algorithm, irreducible edges only, the output of -t 1.  The overlap blocks come from the device, a batch of reads per
// lrsc_overlap_exact call (OverlapProcess.h); the lexicographic order of the reads comes from the index, not from .sai / .rsai.
// -e, -a, -l and -f are not built.  Not taken over: the time stamps.
static const char* OVERLAP_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " overlap [OPTION] ... READSFILE\n"
    "Compute pairwise overlap between all the sequences in READS\n"
    "\n"
    "      --help                           display this help and exit\n"
    "      -v, --verbose                    display verbose output\n"
    "      -t, --threads=NUM                use NUM worker threads to compute the overlaps (default: 1)\n"
    "      -e, --error-rate                 the maximum error rate allowed to consider two sequences aligned (default: 0)\n"
    "      -m, --min-overlap=LEN            minimum overlap required between two reads (default: 45)\n"
    "      -f, --target-file=FILE           perform the overlap queries against the reads in FILE\n"
    "      -a, --algorithm=STR              LSSF: locality-sensitive search by FM-index (default);\n"
    "                                       ADPF: approximate dynamic programming by FM-index\n"
    "      -x, --exhaustive                 output all overlaps, including transitive edges (default if e>0)\n"
    "          --exact                      output irreducible overlaps (default if e=0)\n"
    "      -l, --maxindel                   maximum indels allowed during inexact overlap computation\n"
    "      -p, --prefix=PREFIX              use PREFIX for the names of the index files (default: prefix of the input file)\n"
    "      -o, --outfile=FILE               write the graph to FILE (default: READSFILE.asqg.gz)\n"
    "      --build-index                    index READSFILE in memory on the device instead of loading PREFIX.bwt/.rbwt\n"
    "      --load-on-device                 decode PREFIX.bwt/.rbwt on the device (what loading does here; accepted for symmetry)\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace overlapopt {
static unsigned int verbose = 0;
static int numThreads = 1, sampleRate = 128, device = 0;
static unsigned int minOverlap = 45;
static std::string prefix, readsFile, outFile;
static bool buildIndex = false;
static const size_t batch = 100000;                             // reads per device call
}

static void parseOverlapOptions(int argc, char** argv)
{
    enum { O_HELP = 1, O_VERSION, O_EXACT, O_DEVICE, O_BUILDINDEX, O_LOADONDEVICE };
    static const struct option overlap_longopts[] = {
        {"verbose", no_argument, nullptr, 'v'},               {"threads", required_argument, nullptr, 't'},
        {"min-overlap", required_argument, nullptr, 'm'},     {"sample-rate", required_argument, nullptr, 'd'},
        {"outfile", required_argument, nullptr, 'o'},         {"target-file", required_argument, nullptr, 'f'},
        {"prefix", required_argument, nullptr, 'p'},          {"error-rate", required_argument, nullptr, 'e'},
        {"maxindel", required_argument, nullptr, 'l'},        {"algorithm", required_argument, nullptr, 'a'},
        {"exhaustive", no_argument, nullptr, 'x'},            {"exact", no_argument, nullptr, O_EXACT},
        {"help", no_argument, nullptr, O_HELP},               {"version", no_argument, nullptr, O_VERSION},
        {"device", required_argument, nullptr, O_DEVICE},     {"build-index", no_argument, nullptr, O_BUILDINDEX},
        {"load-on-device", no_argument, nullptr, O_LOADONDEVICE},
        {nullptr, 0, nullptr, 0}};
    optind = 1;
    bool die = false;
    for(int c; (c = getopt_long(argc, argv, "m:d:e:t:l:o:f:a:p:vx", overlap_longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 'm': arg >> overlapopt::minOverlap; break;
            case 'o': arg >> overlapopt::outFile; break;
            case 'p': arg >> overlapopt::prefix; break;
            case 't': arg >> overlapopt::numThreads; break;
            case 'd': arg >> overlapopt::sampleRate; break;
            case 'v': overlapopt::verbose++; break;
            // errorRate stays -1, where the reference turns irreducible-only back on whatever -x said; --exact sets a flag it never reads
            case 'x': case O_EXACT: case O_LOADONDEVICE: break;
            case 'e': case 'a': case 'l': case 'f':
                std::cerr << "overlap: -" << (char)c << " is not built here: only the exact overlap of a reads file with itself is\n";
                die = true;
                break;
            case O_DEVICE: arg >> overlapopt::device; break;
            case O_BUILDINDEX: overlapopt::buildIndex = true; break;
            case O_HELP: std::cout << OVERLAP_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            case O_VERSION: std::cout << "overlap Version " PACKAGE_VERSION " (MI355X back end)\n"; exit(EXIT_SUCCESS);
            default: die = true; break;
        }
    }
    if(argc - optind < 1) { std::cerr << "overlap: missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << "overlap: too many arguments\n"; die = true; }
    if(overlapopt::numThreads <= 0) { std::cerr << "overlap: invalid number of threads: " << overlapopt::numThreads << "\n"; die = true; }
    if((overlapopt::sampleRate & (overlapopt::sampleRate - 1)) != 0) {
        std::cerr << "overlap: invalid parameter to -d/--sample-rate, must be power of 2. got: " << overlapopt::sampleRate << "\n";
        die = true;
    }
    if(die) { std::cout << "\n" << OVERLAP_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    overlapopt::readsFile = argv[optind++];
    if(overlapopt::prefix.empty()) overlapopt::prefix = getFilename(overlapopt::readsFile);
    if(overlapopt::outFile.empty()) overlapopt::outFile = getFilename(overlapopt::readsFile) + ".asqg.gz";
}

static int overlapMain(int argc, char** argv)
{
    parseOverlapOptions(argc, argv);
    const int device = overlapopt::device;
    // ReadInfoTable: the id and the length of every read of the file
    std::vector<std::string> ids;
    std::vector<uint32_t> lengths;
    {
        SeqReader reader(overlapopt::readsFile, true);
        SeqRecord r;
        while(reader.get(r)) { ids.push_back(r.id); lengths.push_back((uint32_t)r.seq.size()); }
    }
    lrsc_index* idx = nullptr;
    if(overlapopt::buildIndex) {
        std::string bases;
        std::vector<uint64_t> off;
        loadReads(overlapopt::readsFile, bases, off);
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)(off.size() - 1), device, &idx), "lrsc_index_build");
    } else {
        std::cout << std::endl << "Loading BWT: " << overlapopt::prefix + BWT_EXT << "\n";
        std::cout << "Loading RBWT: " << overlapopt::prefix + RBWT_EXT << "\n";
        lrscOrDie(lrsc_index_open_device((overlapopt::prefix + BWT_EXT).c_str(), (overlapopt::prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    }
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    if(info.num_strings != ids.size()) {
        std::cerr << "overlap: " << overlapopt::readsFile << " holds " << ids.size() << " reads, the index " << info.num_strings << ": the index is not that of these reads\n";
        lrsc_index_close(idx);
        return EXIT_FAILURE;
    }
    std::vector<uint32_t> order[2];
    for(int rev = 0; rev < 2; ++rev) {
        order[rev].resize(ids.size());
        lrscOrDie(lrsc_index_lexico_order(idx, rev ? LRSC_RBWT : LRSC_BWT, device, order[rev].data(), nullptr), "lrsc_index_lexico_order");
    }
    lrsc_ctx* ctx = nullptr;
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");

    const std::string edgesFile = getFilename(overlapopt::readsFile) + "-thread0.edges.gz";
    gzFile asqg = gzopen(overlapopt::outFile.c_str(), "wb"), edges = gzopen(edgesFile.c_str(), "wb");
    if(!asqg || !edges) { std::cerr << "Error: could not open " << (asqg ? edgesFile : overlapopt::outFile) << " for write\n"; return EXIT_FAILURE; }
    {
        std::ostringstream header;                                // HeaderRecord::write
        header << "HT\tVN:i:1\tER:f:-1\tOL:i:" << overlapopt::minOverlap << "\tIN:Z:" << overlapopt::readsFile << "\tCN:i:1\tTE:i:0\n";
        if(!gzPut(asqg, header.str())) { std::cerr << "Error: could not write " << overlapopt::outFile << "\n"; return EXIT_FAILURE; }
    }
    std::cout << "StriDe overlap computation using min overlap: " << overlapopt::minOverlap << "\n"
              << "Error Rate: -1\n"
              << "Max Indel: 0\n"
              << "Transitive reduction: 1\n"
              << "Algorithm: LSSF\n";
    OverlapParameters params;
    params.ctx = ctx;
    params.minOverlap = (int)overlapopt::minOverlap;
    params.order[0] = &order[0];
    params.order[1] = &order[1];
    params.ids = &ids;
    params.lengths = &lengths;
    bool ok = true;
    {
        OverlapProcess processor(params, edges);
        OverlapPostProcess post(asqg);
        SeqReader reader(overlapopt::readsFile, true);
        WorkItemGenerator<SequenceWorkItem> generator(&reader);
        std::vector<SequenceWorkItem> items;
        std::vector<OverlapResult> results;
        for(bool more = true; more && ok;) {
            items.clear();
            SequenceWorkItem item;
            while(items.size() < overlapopt::batch && (more = generator.generate(item))) items.push_back(item);
            ok = processor.process_batch(items, results);
            for(size_t i = 0; ok && i < items.size(); ++i) ok = post.process(items[i], results[i]);
        }
    }
    ok = (gzclose(asqg) == Z_OK) && ok;
    ok = (gzclose(edges) == Z_OK) && ok;
    std::cout.flush();
    lrsc_ctx_destroy(ctx);
    lrsc_index_close(idx);
    if(!ok) {
        std::cerr << "overlap: the run ended early: " << overlapopt::outFile << " and " << edgesFile << " are not complete\n";
        return EXIT_FAILURE;
    }
    return 0;
}

// `stride fm-merge READSFILE`: the reference's fm-merge (StriDe/fm-merge.cpp:83-220).  Every run of reads that overlap each other
// unambiguously becomes one sequence of PREFIX.merged.fa, all reads in one lrsc_fmmerge call (FMMergeProcess.h).  -t is accepted:
// the device does the work.  Not taken over: the time stamp, printInfo, and the per-graph "<Simplify>" lines.
static const char* FMMERGE_USAGE_MESSAGE =
    "Usage: " PACKAGE_NAME " fm-merge [OPTION] ... READSFILE\n"
    "Merge unambiguously sequences from the READSFILE using the FM-index.\n"
    "This program requires rmdup to be run before it.\n"
    "\n"
    "      --help                           display this help and exit\n"
    "      -v, --verbose                    display verbose output\n"
    "      -p, --prefix=PREFIX              use PREFIX for the names of the index files (default: prefix of the input file)\n"
    "      -t, --threads=NUM                use NUM worker threads (default: no threading)\n"
    "      -m, --min-overlap=LEN            minimum overlap required between two reads to merge (default: 45)\n"
    "      -o, --outfile=FILE               write the merged sequences to FILE (default: basename.merged.fa)\n"
    "      --build-index                    index READSFILE in memory on the device instead of loading PREFIX.bwt/.rbwt\n"
    "      --load-on-device                 decode PREFIX.bwt/.rbwt on the device (what loading does here; accepted for symmetry)\n"
    "      --device=N                       HIP device to work on (default: 0)\n"
    "\nReport bugs to " PACKAGE_BUGREPORT "\n\n";

namespace fmmergeopt {
static unsigned int verbose = 0;
static int numThreads = 1, device = 0;
static unsigned int minOverlap = 45;
static std::string prefix, readsFile, outFile;
static bool buildIndex = false;
}

static void parseFMMergeOptions(int argc, char** argv)
{
    enum { O_HELP = 1, O_VERSION, O_DEVICE, O_BUILDINDEX, O_LOADONDEVICE };
    static const struct option fmmerge_longopts[] = {
        {"prefix", required_argument, nullptr, 'p'},          {"verbose", no_argument, nullptr, 'v'},
        {"threads", required_argument, nullptr, 't'},         {"min-overlap", required_argument, nullptr, 'm'},
        {"outfile", required_argument, nullptr, 'o'},         {"help", no_argument, nullptr, O_HELP},
        {"version", no_argument, nullptr, O_VERSION},         {"device", required_argument, nullptr, O_DEVICE},
        {"build-index", no_argument, nullptr, O_BUILDINDEX},  {"load-on-device", no_argument, nullptr, O_LOADONDEVICE},
        {nullptr, 0, nullptr, 0}};
    optind = 1;
    bool die = false;
    for(int c; (c = getopt_long(argc, argv, "p:m:d:e:t:l:s:o:vix", fmmerge_longopts, nullptr)) != -1;) {
        std::istringstream arg(optarg != nullptr ? optarg : "");
        switch(c) {
            case 'm': arg >> fmmergeopt::minOverlap; break;
            case 'p': arg >> fmmergeopt::prefix; break;
            case 'o': arg >> fmmergeopt::outFile; break;
            case 't': arg >> fmmergeopt::numThreads; break;
            case '?': die = true; break;
            case 'v': fmmergeopt::verbose++; break;
            case O_DEVICE: arg >> fmmergeopt::device; break;
            case O_BUILDINDEX: fmmergeopt::buildIndex = true; break;
            case O_LOADONDEVICE: break;
            case O_HELP: std::cout << FMMERGE_USAGE_MESSAGE; exit(EXIT_SUCCESS);
            case O_VERSION: std::cout << "fm-merge Version " PACKAGE_VERSION " (MI355X back end)\n"; exit(EXIT_SUCCESS);
            default: break;                                       // d, e, l, s, i, x: in the reference's option string, read by nothing
        }
    }
    if(argc - optind < 1) { std::cerr << "fm-merge: missing arguments\n"; die = true; }
    else if(argc - optind > 1) { std::cerr << "fm-merge: too many arguments\n"; die = true; }
    if(fmmergeopt::numThreads <= 0) { std::cerr << "fm-merge: invalid number of threads: " << fmmergeopt::numThreads << "\n"; die = true; }
    if(die) { std::cout << "\n" << FMMERGE_USAGE_MESSAGE; exit(EXIT_FAILURE); }
    fmmergeopt::readsFile = argv[optind++];
    if(fmmergeopt::prefix.empty()) fmmergeopt::prefix = getFilename(fmmergeopt::readsFile);
    if(fmmergeopt::outFile.empty()) fmmergeopt::outFile = fmmergeopt::prefix + ".merged.fa";
}

static int fmmergeMain(int argc, char** argv)
{
    parseFMMergeOptions(argc, argv);
    const int device = fmmergeopt::device;
    std::string bases;
    std::vector<uint64_t> off;
    loadReads(fmmergeopt::readsFile, bases, off);
    const size_t numReads = off.size() - 1;
    lrsc_index* idx = nullptr;
    if(fmmergeopt::buildIndex) {
        lrscOrDie(lrsc_index_build(bases.data(), off.data(), (uint32_t)numReads, device, &idx), "lrsc_index_build");
    } else {
        std::cout << std::endl << "Loading BWT: " << fmmergeopt::prefix + BWT_EXT << "\n";
        std::cout << "Loading RBWT: " << fmmergeopt::prefix + RBWT_EXT << "\n";
        lrscOrDie(lrsc_index_open_device((fmmergeopt::prefix + BWT_EXT).c_str(), (fmmergeopt::prefix + RBWT_EXT).c_str(), device, &idx), "lrsc_index_open_device");
    }
    lrsc_index_info info;
    lrscOrDie(lrsc_index_info_get(idx, &info), "lrsc_index_info_get");
    if(info.num_strings != numReads) {
        std::cerr << "fm-merge: " << fmmergeopt::readsFile << " holds " << numReads << " reads, the index " << info.num_strings << ": the index is not that of these reads\n";
        lrsc_index_close(idx);
        return EXIT_FAILURE;
    }
    lrsc_ctx* ctx = nullptr;
    lrscOrDie(lrsc_ctx_create(idx, nullptr, device, &ctx), "lrsc_ctx_create");
    printf("[%s::fm-merge] starting read merging on device %d\n", PACKAGE_NAME, device);
    bool ok = true;
    {
        stride::FMMergeProcess processor(ctx, (int)fmmergeopt::minOverlap);
        stride::FMMergeResult result;
        ok = processor.process(bases, off, result);
        if(ok) {
            std::ofstream writer(fmmergeopt::outFile.c_str());
            if(!writer) { std::cerr << "Error: could not open " << fmmergeopt::outFile << " for write\n"; ok = false; }
            else {
                stride::FMMergePostProcess post(&writer);
                ok = post.process(result);
                writer.flush();
                ok = ok && (bool)writer;
            }
        }
    }
    fflush(stdout);
    lrsc_ctx_destroy(ctx);
    lrsc_index_close(idx);
    if(!ok) {
        std::cerr << "fm-merge: the run ended early: " << fmmergeopt::outFile << " is not complete\n";
        return EXIT_FAILURE;
    }
    return 0;
}

int main(int argc, char** argv)
{
    // several workers on one device (--devices 0,0) only overlap if their streams get hardware queues of their own (default: 4)
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    if(argc <= 1) { std::cerr << "Usage: " PACKAGE_NAME " <command> [options]\nCommands: index, merge, sai, grep, filter, correct, pbcorrect, kmerfreq, kmercheck\n          and fmwalk\n          and overlap\n          and fm-merge\n"; return EXIT_FAILURE; }
    const std::string command(argv[1]);
    if(command == "help" || command == "--help") { std::cout << "Usage: " PACKAGE_NAME " <command> [options]\nCommands: index, merge, sai, grep, filter, correct, pbcorrect, kmerfreq, kmercheck\n          and fmwalk\n          and overlap\n          and fm-merge\n"; return 0; }
    if(command == "pbcorrect" || command == SUBPROGRAM) return PacBioSelfCorrectionMain(argc - 1, argv + 1);
    if(command == "index") return indexMain(argc - 1, argv + 1);
    if(command == "merge") return mergeMain(argc - 1, argv + 1);
    if(command == "sai") return saiMain(argc - 1, argv + 1);
    if(command == "grep") return grepMain(argc - 1, argv + 1);
    if(command == "filter") return filterMain(argc - 1, argv + 1);
    if(command == "correct") return correctMain(argc - 1, argv + 1);
    if(command == "fmwalk") return fmwalkMain(argc - 1, argv + 1);
    if(command == "overlap") return overlapMain(argc - 1, argv + 1);
    if(command == "fm-merge") return fmmergeMain(argc - 1, argv + 1);
    if(command == "kmerfreq") return kmerfreqMain(argc - 1, argv + 1);
    if(command == "kmercheck") return kmercheckMain(argc - 1, argv + 1);
    std::cerr << "Unrecognized command: " << command << "\n";
    return EXIT_FAILURE;
}
