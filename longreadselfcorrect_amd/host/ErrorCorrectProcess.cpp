// ErrorCorrectProcess.cpp -- see ErrorCorrectProcess.h (reference behaviour: Algorithm/ErrorCorrectProcess.cpp:287-438,550-676,
// Util/Metrics.h:42-52, Util/Util.h:76-91).
#include "ErrorCorrectProcess.h"

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

std::vector<ErrorCorrectResult> ErrorCorrectProcess::process_batch(const std::vector<SequenceWorkItem>& items)
{
    std::vector<ErrorCorrectResult> results(items.size());
    std::string bases;
    std::vector<uint8_t> phred;
    std::vector<uint64_t> off(1, 0);
    std::vector<size_t> sent;                                     // the reads that go to the device
    bool any_qual = false;
    for(size_t n = 0; n < items.size(); ++n) {
        const SeqRecord& r = items[n].read;
        if(!r.qual.empty()) {
            bool ok = r.qual.size() == r.seq.size();
            for(size_t i = 0; ok && i < r.qual.size(); ++i) ok = r.qual[i] >= '!';
            if(!ok) {
                std::cerr << "correct: read " << r.id << " of " << m_params.readsFile << " has a quality string of " << r.qual.size() << " characters for "
                          << r.seq.size() << " bases, or a quality character below '!'\n";
                exit(EXIT_FAILURE);
            }
        }
        results[n].correctSequence = r.seq;                       // what a read that is not corrected keeps
        if(r.seq.empty()) continue;
        if(!onlyACGT(r.seq)) {
            if(!m_warnedOtherBases)
                std::cerr << "Warning: read " << r.id << " holds a base other than A, C, G, T: such reads are written as they are and fail QC\n";
            m_warnedOtherBases = true;
            continue;
        }
        sent.push_back(n);
        bases += r.seq;
        off.push_back(bases.size());
        // getPhredScore: the character - 33, 15 for a read without qualities
        for(size_t i = 0; i < r.seq.size(); ++i) phred.push_back(r.qual.empty() ? 15 : (uint8_t)(r.qual[i] - 33));
        any_qual |= !r.qual.empty();
    }
    if(sent.empty()) return results;
    lrsc_kcorrect_params p;
    p.kmer_length = m_params.kmerLength;
    p.kmer_threshold = m_params.kmerThreshold;
    p.kmer_rounds = m_params.numKmerRounds;
    p.quality_cutoff = m_params.highQualityCutoff;
    std::string corrected(bases.size(), '\0');
    std::vector<lrsc_kcorrect_result> res(sent.size());
    orDie(lrsc_kmer_correct(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), any_qual ? phred.data() : nullptr, &p, &corrected[0], res.data()),
          "lrsc_kmer_correct");
    for(size_t q = 0; q < sent.size(); ++q) {
        results[sent[q]].correctSequence = corrected.substr(off[q], off[q + 1] - off[q]);
        results[sent[q]].kmerQC = res[q].kmer_qc != 0;
    }
    return results;
}

template <class Key>
void ErrorCountMap<Key>::write(std::ostream* pWriter, const std::string& leader, const std::string& header) const
{
    *pWriter << leader;
    *pWriter << header << "\tsamples\terrors\tfraction\n";
    for(typename std::map<Key, ErrorCount>::const_iterator iter = m_data.begin(); iter != m_data.end(); ++iter)
        *pWriter << iter->first << "\t" << iter->second.num_samples << "\t" << iter->second.num_errors << "\t"
                 << (double)iter->second.num_errors / iter->second.num_samples << "\n";
}

ErrorCorrectPostProcess::ErrorCorrectPostProcess(std::ostream* pCorrectedWriter, std::ostream* pDiscardWriter, bool bCollectMetrics)
    : m_pCorrectedWriter(pCorrectedWriter), m_pDiscardWriter(pDiscardWriter), m_bCollectMetrics(bCollectMetrics)
{
}

ErrorCorrectPostProcess::~ErrorCorrectPostProcess()
{
    std::cout << "Reads passed kmer QC check: " << m_kmerQCPassed << "\n";
    std::cout << "Reads passed overlap QC check: " << m_overlapQCPassed << "\n";
    std::cout << "Reads failed QC: " << m_qcFail << "\n";
}

void ErrorCorrectPostProcess::writeMetrics(std::ostream* pWriter)
{
    m_positionMetrics.write(pWriter, "Bases corrected by position\n", "pos");
    m_originalBaseMetrics.write(pWriter, "\nOriginal base that was corrected\n", "base");
    m_precedingSeqMetrics.write(pWriter, "\nkmer preceding the corrected base\n", "kmer");
    m_qualityMetrics.write(pWriter, "\nBases corrected by quality value\n\n", "quality");
    std::cout << "ErrorCorrect -- Corrected " << m_totalErrors << " out of " << m_totalBases << " bases (" << (double)m_totalErrors / m_totalBases << ")\n";
    std::cout << "Kept " << m_readsKept << " reads. Discarded " << m_readsDiscarded << " reads ("
              << (double)m_readsDiscarded / (m_readsKept + m_readsDiscarded) << ")\n";
}

// SeqRecord::write: FASTQ when the record has qualities, else FASTA
static void writeRecord(std::ostream& out, const SeqRecord& r, const std::string& seq)
{
    if(!r.qual.empty()) out << "@" << r.id << "\n" << seq << "\n+\n" << r.qual << "\n";
    else out << ">" << r.id << "\n" << seq << "\n";
}

void ErrorCorrectPostProcess::process(const SequenceWorkItem& item, const ErrorCorrectResult& result)
{
    bool readQCPass = true;
    if(result.kmerQC) m_kmerQCPassed += 1;
    else if(result.overlapQC) m_overlapQCPassed += 1;
    else {
        readQCPass = false;
        m_qcFail += 1;
    }
    // metrics are collected for the reads that were actually corrected
    if(m_bCollectMetrics && readQCPass) collectMetrics(item.read.seq, result.correctSequence, item.read.qual);
    if(result.correctSequence.empty()) return;
    if(readQCPass || m_pDiscardWriter == nullptr) {
        writeRecord(*m_pCorrectedWriter, item.read, result.correctSequence);
        ++m_readsKept;
    } else {
        writeRecord(*m_pDiscardWriter, item.read, result.correctSequence);
        ++m_readsDiscarded;
    }
}

void ErrorCorrectPostProcess::collectMetrics(const std::string& originalSeq, const std::string& correctedSeq, const std::string& qualityStr)
{
    const size_t precedingLen = 2;
    for(size_t i = 0; i < originalSeq.length(); ++i) {
        const char qc = !qualityStr.empty() ? qualityStr[i] : '\0';
        const char ob = originalSeq[i];
        ++m_totalBases;
        m_positionMetrics.incrementSample((int64_t)i);
        if(!qualityStr.empty()) m_qualityMetrics.incrementSample(qc);
        m_originalBaseMetrics.incrementSample(ob);
        std::string precedingMer;
        if(i > precedingLen) {                                    // the reference's test: the 2-mer before base 2 is never taken
            precedingMer = originalSeq.substr(i - precedingLen, precedingLen);
            m_precedingSeqMetrics.incrementSample(precedingMer);
        }
        if(originalSeq[i] != correctedSeq[i]) {
            m_positionMetrics.incrementError((int64_t)i);
            if(!qualityStr.empty()) m_qualityMetrics.incrementError(qc);
            m_originalBaseMetrics.incrementError(ob);
            if(!precedingMer.empty()) m_precedingSeqMetrics.incrementError(precedingMer);
            ++m_totalErrors;
        }
    }
}

} // namespace stride
