// FMIndexWalkProcess.cpp -- see FMIndexWalkProcess.h (reference behaviour: FMIndexWalk/FMIndexWalkProcess.cpp:153-226, 898-920,
// 972-1020, Util/Util.h:76-91).
#include "FMIndexWalkProcess.h"

#include <algorithm>
#include <cstdlib>
#include <iostream>

namespace stride {

static void orDie(int st, const char* what)
{
    if(st != LRSC_OK) {
        std::cerr << what << ": " << lrsc_strerror(st) << " (" << lrsc_last_error() << ")\n";
        exit(EXIT_FAILURE);
    }
}

static bool onlyACGT(const std::string& s)
{
    for(size_t i = 0; i < s.size(); ++i)
        if(s[i] != 'A' && s[i] != 'C' && s[i] != 'G' && s[i] != 'T') return false;
    return true;
}

std::vector<FMIndexWalkResult> FMIndexWalkProcess::process_batch(const std::vector<SequenceWorkItemPair>& pairs)
{
    std::vector<FMIndexWalkResult> results(pairs.size());
    std::string bases;
    std::vector<uint64_t> off(1, 0);
    std::vector<size_t> sent;                                     // the pairs that go to the device
    for(size_t n = 0; n < pairs.size(); ++n) {
        const std::string& s1 = pairs[n].first.read.seq;
        const std::string& s2 = pairs[n].second.read.seq;
        if(s1.empty() || s2.empty()) continue;
        if(!onlyACGT(s1) || !onlyACGT(s2)) {
            if(!m_warnedOtherBases)
                std::cerr << "Warning: pair " << pairs[n].first.read.id << " holds a base other than A, C, G, T: such pairs are not merged\n";
            m_warnedOtherBases = true;
            continue;
        }
        sent.push_back(n);
        bases += s1;
        off.push_back(bases.size());
        bases += s2;
        off.push_back(bases.size());
    }
    if(sent.empty()) return results;
    lrsc_fmwalk_params p;
    p.kmer_length = m_params.kmerLength;
    p.kmer_threshold = m_params.kmerThreshold;
    p.min_overlap = m_params.minOverlap;
    p.max_overlap = m_params.maxOverlap;
    p.max_insert = m_params.maxInsertSize;
    p.max_leaves = m_params.maxLeaves;
    const uint64_t stride = (uint64_t)std::max(std::max(p.max_insert + 1, p.min_overlap), 1);
    std::string merged(sent.size() * stride, '\0');
    std::vector<lrsc_fmwalk_result> res(sent.size());
    orDie(lrsc_fmwalk_merge(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), &p, &merged[0], stride, res.data()), "lrsc_fmwalk_merge");
    for(size_t q = 0; q < sent.size(); ++q) {
        if(!res[q].merged) continue;
        results[sent[q]].merge = true;
        results[sent[q]].correctSequence = merged.substr(q * stride, res[q].length);
    }
    return results;
}

FMIndexWalkPostProcess::~FMIndexWalkPostProcess()
{
    std::cout << "Reads are kmerized: " << m_kmerizePassed << "\n";
    std::cout << "Reads are merged : " << m_mergePassed << "\n";
    std::cout << "Reads failed to kmerize or merge: " << m_qcFail << "\n";
}

void FMIndexWalkPostProcess::process(const SequenceWorkItemPair& itemPair, const FMIndexWalkResult& result)
{
    if(!result.merge) {
        m_qcFail += 2;
        return;
    }
    m_mergePassed += 1;
    const std::string& id = itemPair.first.read.id;
    *m_pCorrectedWriter << ">" << id.substr(0, id.find('/')) << "\n" << result.correctSequence << "\n";      // SeqItem::write
}

} // namespace stride
