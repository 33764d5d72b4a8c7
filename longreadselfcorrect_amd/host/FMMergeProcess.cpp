// FMMergeProcess.cpp -- see FMMergeProcess.h
#include "FMMergeProcess.h"

#include <cstdio>
#include <iostream>

namespace stride {

bool FMMergeProcess::process(const std::string& bases, const std::vector<uint64_t>& off, FMMergeResult& result)
{
    const uint32_t n = (uint32_t)(off.size() - 1);
    result.reads.assign(n, lrsc_fmmerge_read{0, 0, 0});
    result.seqs.assign(n, lrsc_fmmerge_seq{0, 0, 0, 0, 0, 0});
    // no sequence set is longer than its reads back to back
    result.bases.assign(bases.size(), '\0');
    uint32_t n_seqs = 0;
    uint64_t n_bases = 0;
    const int st = lrsc_fmmerge(m_ctx, bases.data(), off.data(), n, m_minOverlap, result.reads.data(), result.seqs.data(), &n_seqs, &result.bases[0], result.bases.size(),
                                &n_bases);
    if(st != LRSC_OK) {
        std::cerr << "fm-merge: " << lrsc_strerror(st) << " (" << lrsc_last_error() << ")\n";
        return false;
    }
    result.seqs.resize(n_seqs);
    result.bases.resize(n_bases);
    return true;
}

bool FMMergePostProcess::process(const FMMergeResult& result)
{
    m_numTotal += result.reads.size();
    for(const lrsc_fmmerge_seq& s : result.seqs) {
        *m_writer << ">merged-" << m_numMerged++ << "\n";         // SeqRecord::write of a record without qualities
        m_writer->write(result.bases.data() + s.offset, (std::streamsize)s.length);
        *m_writer << "\n";
        m_totalLength += s.length;
    }
    return (bool)*m_writer;
}

FMMergePostProcess::~FMMergePostProcess()
{
    printf("[sga fm-merge] Merged %zu reads into %zu sequences\n", m_numTotal, m_numMerged);
    printf("[sga fm-merge] Reduction factor: %lf\n", (double)m_numTotal / m_numMerged);
    printf("[sga fm-merge] Mean merged size: %lf\n", (double)m_totalLength / m_numMerged);
}

} // namespace stride
