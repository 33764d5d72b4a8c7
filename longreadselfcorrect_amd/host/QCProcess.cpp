// QCProcess.cpp -- see QCProcess.h (reference behaviour: Algorithm/QCProcess.cpp:54-88,268-441).
#include "QCProcess.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>

namespace stride {

static void orDie(int st, const char* what)
{
    if(st != LRSC_OK) {
        std::cerr << what << ": " << lrsc_strerror(st) << " (" << lrsc_last_error() << ")\n";
        exit(EXIT_FAILURE);
    }
}

std::vector<QCResult> QCProcess::process_batch(const std::vector<SequenceWorkItem>& items, std::vector<lrsc_dup_result>* dup)
{
    std::vector<QCResult> results(items.size());
    if(items.empty()) return results;
    std::string bases;
    std::vector<uint64_t> off(1, 0);
    for(const SequenceWorkItem& it : items) { bases += it.read.seq; off.push_back(bases.size()); }
    std::vector<lrsc_dup_result> records(items.size());
    orDie(lrsc_dupcheck_reads(m_params.dupcheck, bases.data(), off.data(), (uint32_t)items.size(), records.data()), "lrsc_dupcheck_reads");
    if(m_params.checkDuplicates)
        for(size_t i = 0; i < items.size(); ++i)
            results[i].dupPassed = m_params.substringOnly ? records[i].cls != LRSC_DUP_SUBSTRING : records[i].cls == LRSC_DUP_UNIQUE;
    // the k-mer check would come here, for the reads that passed so far; `stride filter` never asks for it
    if(m_params.checkHPRuns) homopolymerCheck(items, results);
    if(m_params.checkDegenerate)
        for(size_t i = 0; i < items.size(); ++i)
            if(results[i].passed()) results[i].degenPassed = degenerateCheck(items[i]);
    if(dup) dup->swap(records);
    return results;
}

// performHomopolymerCheck for the reads that passed so far.  The k-mer that covers a read's longest run is counted with the run
// 2 shorter to 2 longer; the composites of all reads of one length go to the device in one lrsc_find_kmers call.
void QCProcess::homopolymerCheck(const std::vector<SequenceWorkItem>& items, std::vector<QCResult>& results)
{
    const size_t k = m_params.hpKmerLength;
    struct Candidate { size_t item, maxRunLength; char runChar; std::string prefix, suffix; size_t count[5]; };
    std::vector<Candidate> cands;
    for(size_t n = 0; n < items.size(); ++n) {
        if(!(results[n].kmerPassed && results[n].dupPassed)) continue;
        const std::string& w = items[n].read.seq;
        if(w.size() < k) continue;
        // the first of the longest runs of one base
        size_t run_len = 0, run_start = 0;
        for(size_t i = 0, j; i < w.size(); i = j) {
            for(j = i + 1; j < w.size() && w[j] == w[i]; ++j) {}
            if(j - i > run_len) { run_len = j - i; run_start = i; }
        }
        if(run_len < m_params.hpMinLength || run_len >= k / 2) continue;
        // the k-mer centred on the run, moved inside the read where it would stick out
        const long centred = (long)(run_start + run_len / 2) - (long)(k / 2);
        size_t kmer_start = centred < 0 ? 0 : (size_t)centred;
        if(centred + (long)k > (long)w.size()) kmer_start = w.size() - k;
        Candidate c;
        c.item = n; c.maxRunLength = run_len; c.runChar = w[run_start];
        c.prefix = w.substr(kmer_start, run_start - kmer_start);
        c.suffix = w.substr(run_start + run_len, kmer_start + k - (run_start + run_len));
        // no verdict without enough context on either side of the run
        if(c.prefix.size() < m_params.hpMinContext || c.suffix.size() < m_params.hpMinContext) continue;
        cands.push_back(c);
    }
    // countSequenceOccurrences: the occurrences of the composite plus those of its reverse complement
    std::map<size_t, std::vector<std::pair<size_t, int> > > by_len;       // composite length -> (candidate, which of the five)
    for(size_t j = 0; j < cands.size(); ++j)
        for(int d = 0; d < 5; ++d) by_len[cands[j].prefix.size() + cands[j].suffix.size() + cands[j].maxRunLength - 2 + (size_t)d].push_back(std::make_pair(j, d));
    for(std::map<size_t, std::vector<std::pair<size_t, int> > >::const_iterator kv = by_len.begin(); kv != by_len.end(); ++kv) {
        std::string kmers;
        for(size_t q = 0; q < kv->second.size(); ++q) {
            const Candidate& c = cands[kv->second[q].first];
            kmers += c.prefix + std::string(c.maxRunLength - 2 + (size_t)kv->second[q].second, c.runChar) + c.suffix;
        }
        std::vector<lrsc_biinterval> iv(kv->second.size());
        orDie(lrsc_find_kmers(m_params.ctx, kmers.data(), (uint32_t)kv->first, iv.size(), iv.data()), "lrsc_find_kmers");
        for(size_t q = 0; q < iv.size(); ++q) {
            const lrsc_biinterval& b = iv[q];
            cands[kv->second[q].first].count[kv->second[q].second] = (size_t)((b.fwd.lower <= b.fwd.upper ? b.fwd.upper - b.fwd.lower + 1 : 0) +
                                                                              (b.rvc.lower <= b.rvc.upper ? b.rvc.upper - b.rvc.lower + 1 : 0));
        }
    }
    for(size_t j = 0; j < cands.size(); ++j) {
        const Candidate& c = cands[j];
        size_t highestCountLength = 0, highestCount = 0;
        const size_t actualCount = c.count[2];
        for(int d = 0; d < 5; ++d)
            if(c.count[d] > highestCount) { highestCount = c.count[d]; highestCountLength = c.maxRunLength - 2 + (size_t)d; }
        const double proportion = (double)actualCount / (double)highestCount;
        if(highestCountLength == c.maxRunLength || actualCount >= m_params.hpHardAcceptCount || proportion >= m_params.hpMinProportion) continue;
        if(m_params.verbose > 0) {
            printf("Read failed homopolymer filter %s\n", items[c.item].read.seq.c_str());
            printf("Filtered read with poly-%c run. DL: %zu DC: %zu. AL: %zu AC: %zu P: %lf\n", c.runChar, highestCountLength, highestCount, c.maxRunLength,
                   actualCount, proportion);
        }
        results[c.item].hpPassed = false;
    }
}

// performDegenerateCheck: false when one base makes up more than degenProportion of the read
bool QCProcess::degenerateCheck(const SequenceWorkItem& item) const
{
    const std::string& w = item.read.seq;
    size_t bc[256] = {0};
    for(size_t i = 0; i < w.size(); ++i) bc[(unsigned char)w[i]] += 1;
    const size_t maxCount = std::max(std::max(bc[(int)'A'], bc[(int)'C']), std::max(bc[(int)'G'], bc[(int)'T']));
    const double prop = (double)maxCount / w.size();
    if(prop > m_params.degenProportion) {
        if(m_params.verbose > 0) std::cout << "Read " << w << " failed degenerate filter\n";
        return false;
    }
    return true;
}

QCPostProcess::QCPostProcess(std::ostream* pCorrectedWriter, std::ostream* pDiscardWriter)
    : m_pCorrectedWriter(pCorrectedWriter), m_pDiscardWriter(pDiscardWriter)
{
}

QCPostProcess::~QCPostProcess()
{
    std::cout << "Reads kept: " << m_readsKept << "\n";
    std::cout << "Reads discarded: " << m_readsDiscarded << "\n";
    std::cout << "Reads failed kmer check: " << m_readsFailedKmer << "\n";
    std::cout << "Reads failed duplicate check: " << m_readsFailedDup << "\n";
    std::cout << "Reads failed homopolymer check: " << m_readsFailedHP << "\n";
    std::cout << "Reads failed degenerate check: " << m_readsFailedDegen << "\n";
}

// SeqRecord::write (Util/Util.h:77-91): FASTQ when there is a quality string, else FASTA
static void writeRecord(std::ostream& out, const std::string& id, const SeqRecord& r)
{
    if(!r.qual.empty()) out << "@" << id << "\n" << r.seq << "\n+\n" << r.qual << "\n";
    else out << ">" << id << "\n" << r.seq << "\n";
}

void QCPostProcess::process(const SequenceWorkItem& item, const QCResult& result)
{
    if(result.passed()) {
        writeRecord(*m_pCorrectedWriter, item.read.id, item.read);
        ++m_readsKept;
        return;
    }
    // the position in the original reads file goes into the name of a discarded read
    std::stringstream newID;
    newID << item.read.id << ",seqrank=" << item.idx;
    writeRecord(*m_pDiscardWriter, newID.str(), item.read);
    ++m_readsDiscarded;
    if(!result.kmerPassed) m_readsFailedKmer += 1;
    else if(!result.dupPassed) m_readsFailedDup += 1;
    else if(!result.hpPassed) m_readsFailedHP += 1;
    else if(!result.degenPassed) m_readsFailedDegen += 1;
}

} // namespace stride
