// FMIndexWalkProcess.cpp -- see FMIndexWalkProcess.h (reference behaviour: FMIndexWalk/FMIndexWalkProcess.cpp:29-150, 153-226,
// 229-267, 269-391, 898-1020, Util/Util.h:51-98).
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

// the slots of the reads' pieces as lrsc_fmwalk_kmerize and lrsc_fmwalk_hybrid place them
static std::vector<uint64_t> pieceSlots(const std::vector<uint64_t>& off, int kmerLength)
{
    std::vector<uint64_t> slot(off.size(), 0);
    const uint64_t k = (uint64_t)std::max(kmerLength, 1);
    for(size_t i = 0; i + 1 < off.size(); ++i) {
        const uint64_t len = off[i + 1] - off[i];
        slot[i + 1] = slot[i] + (len >= k ? len - k + 1 : 0);
    }
    return slot;
}

// correctSequence and kmerizedReads of one read from its record and pieces (FMIndexWalkProcess.cpp:126-135, 255-264)
static void takePieces(const std::string& read, const lrsc_fmwalk_read_result& r, const lrsc_fmwalk_piece* pieces, std::string& correct,
                       std::vector<std::string>& kmerized)
{
    if(r.whole) correct = read.substr((size_t)r.head, r.length);
    for(uint32_t i = 0; i < r.n_pieces; ++i) {
        if(!pieces[i].kept) continue;
        if((int32_t)i == r.main_piece) correct = read.substr(pieces[i].start, pieces[i].length);
        else kmerized.push_back(read.substr(pieces[i].start, pieces[i].length));
    }
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
    if(m_params.algorithm == FMW_HYBRID) {
        const std::vector<uint64_t> slot = pieceSlots(off, p.kmer_length);
        std::vector<lrsc_fmwalk_hybrid_result> res(sent.size());
        std::vector<lrsc_fmwalk_piece> pieces(std::max<uint64_t>(slot.back(), 1));
        orDie(lrsc_fmwalk_hybrid(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), &p, m_params.repeatKmerFreq, &merged[0], stride, res.data(), pieces.data(),
                                 slot.back()),
              "lrsc_fmwalk_hybrid");
        for(size_t q = 0; q < sent.size(); ++q) {
            FMIndexWalkResult& out = results[sent[q]];
            out.kmerize = res[q].read[0].kmerize != 0;
            out.kmerize2 = res[q].read[1].kmerize != 0;
            if(res[q].walk.merged) {
                out.merge = true;
                out.correctSequence = merged.substr(q * stride, res[q].walk.length);
                continue;
            }
            takePieces(pairs[sent[q]].first.read.seq, res[q].read[0], pieces.data() + slot[2 * q], out.correctSequence, out.kmerizedReads);
            takePieces(pairs[sent[q]].second.read.seq, res[q].read[1], pieces.data() + slot[2 * q + 1], out.correctSequence2, out.kmerizedReads2);
        }
        return results;
    }
    std::vector<lrsc_fmwalk_result> res(sent.size());
    orDie(lrsc_fmwalk_merge(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), &p, &merged[0], stride, res.data()), "lrsc_fmwalk_merge");
    for(size_t q = 0; q < sent.size(); ++q) {
        if(!res[q].merged) continue;
        results[sent[q]].merge = true;
        results[sent[q]].correctSequence = merged.substr(q * stride, res[q].length);
    }
    return results;
}

std::vector<FMIndexWalkResult> FMIndexWalkProcess::process_batch(const std::vector<SequenceWorkItem>& reads)
{
    std::vector<FMIndexWalkResult> results(reads.size());
    std::string bases;
    std::vector<uint64_t> off(1, 0);
    std::vector<size_t> sent;
    for(size_t n = 0; n < reads.size(); ++n) {
        const std::string& s = reads[n].read.seq;
        if(s.empty()) continue;
        if(!onlyACGT(s)) {
            if(!m_warnedOtherBases) std::cerr << "Warning: read " << reads[n].read.id << " holds a base other than A, C, G, T: such reads are not kmerized\n";
            m_warnedOtherBases = true;
            continue;
        }
        sent.push_back(n);
        bases += s;
        off.push_back(bases.size());
    }
    if(sent.empty()) return results;
    const std::vector<uint64_t> slot = pieceSlots(off, m_params.kmerLength);
    if(m_params.algorithm == FMW_VALIDATE) {
        size_t longest = 0;
        for(size_t q = 0; q < sent.size(); ++q) {
            const SeqRecord& r = reads[sent[q]].read;
            // a walk's string is at most one base longer than its depth limit, (size_t)(length * 1.1)
            if((size_t)((double)r.seq.size() * 1.1) + 1 > LRSC_FMWALK_MAX_INSERT) {
                std::cerr << "FMIndexWalk: read " << r.id << " has " << r.seq.size() << " bases: --validate takes reads whose walks leave at most "
                          << LRSC_FMWALK_MAX_INSERT << "\n";
                exit(EXIT_FAILURE);
            }
            longest = std::max(longest, r.seq.size());
        }
        lrsc_fmwalk_params p;
        p.kmer_length = m_params.kmerLength;
        p.kmer_threshold = m_params.kmerThreshold;
        p.min_overlap = m_params.minOverlap;
        p.max_overlap = m_params.maxOverlap;
        p.max_insert = 0;                                         // not used: the depth limit is the read's
        p.max_leaves = m_params.maxLeaves;
        const uint64_t stride = (uint64_t)((double)longest * 1.1) + 1;
        std::string merged(sent.size() * stride, '\0');
        std::vector<lrsc_fmwalk_validate_result> res(sent.size());
        std::vector<lrsc_fmwalk_piece> pieces(std::max<uint64_t>(slot.back(), 1));
        orDie(lrsc_fmwalk_validate(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), &p, &merged[0], stride, res.data(), pieces.data(), slot.back()),
              "lrsc_fmwalk_validate");
        for(size_t q = 0; q < sent.size(); ++q) {
            FMIndexWalkResult& out = results[sent[q]];
            out.kmerize = res[q].read.kmerize != 0;
            if(res[q].merged) {
                out.merge = true;
                out.correctSequence = merged.substr(q * stride, res[q].length);
                continue;
            }
            takePieces(reads[sent[q]].read.seq, res[q].read, pieces.data() + slot[q], out.correctSequence, out.kmerizedReads);
        }
        return results;
    }
    std::vector<lrsc_fmwalk_read_result> res(sent.size());
    std::vector<lrsc_fmwalk_piece> pieces(std::max<uint64_t>(slot.back(), 1));
    orDie(lrsc_fmwalk_kmerize(m_params.ctx, bases.data(), off.data(), (uint32_t)sent.size(), m_params.kmerLength, m_params.kmerThreshold, res.data(), pieces.data(),
                              slot.back()),
          "lrsc_fmwalk_kmerize");
    for(size_t q = 0; q < sent.size(); ++q) {
        FMIndexWalkResult& out = results[sent[q]];
        out.kmerize = res[q].kmerize != 0;
        takePieces(reads[sent[q]].read.seq, res[q], pieces.data() + slot[q], out.correctSequence, out.kmerizedReads);
    }
    return results;
}

FMIndexWalkPostProcess::~FMIndexWalkPostProcess()
{
    std::cout << "Reads are kmerized: " << m_kmerizePassed << "\n";
    std::cout << "Reads are merged : " << m_mergePassed << "\n";
    std::cout << "Reads failed to kmerize or merge: " << m_qcFail << "\n";
}

// SeqRecord::write (Util/Util.h:77-91): FASTQ when the record has a quality string, whatever the sequence's length
static void writeRecord(std::ostream& out, const SeqRecord& record, const std::string& seq)
{
    if(!record.qual.empty()) out << "@" << record.id << "\n" << seq << "\n+\n" << record.qual << "\n";
    else out << ">" << record.id << "\n" << seq << "\n";
}
// what the discard writer gets of one read: its correctSequence under its own id, the kmerizedReads as `>id:i` FASTA
// (SeqRecord::writeFasta, Util/Util.h:93-98)
static void writeKmerized(std::ostream& out, const SeqRecord& record, const std::string& correct, const std::vector<std::string>& kmerized)
{
    if(!correct.empty()) writeRecord(out, record, correct);
    for(size_t i = 0; i < kmerized.size(); ++i) out << ">" << record.id << ":" << i << "\n" << kmerized[i] << "\n";
}

// FMIndexWalkProcess.cpp:922-969 for the kmerize and validate algorithms.  In kmerize mode a read that is not kmerized is counted
// and not written: the reference writes it to a writer that only the validate algorithm opens.  In validate mode a merged read goes
// to the corrected writer as FASTA (SeqItem::write), a kmerized one to the discard writer, any other, with its correctSequence,
// to LowComplexityReads.fa.
void FMIndexWalkPostProcess::process(const SequenceWorkItem& item, const FMIndexWalkResult& result)
{
    if(result.kmerize) m_kmerizePassed += 1;
    else if(result.merge) m_mergePassed += 1;
    else m_qcFail += 1;
    if(result.merge) *m_pCorrectedWriter << ">" << item.read.id << "\n" << result.correctSequence << "\n";
    else if(result.kmerize && m_pDiscardWriter != nullptr) writeKmerized(*m_pDiscardWriter, item.read, result.correctSequence, result.kmerizedReads);
    else if(!result.kmerize && m_pLowComplexWriter != nullptr) writeRecord(*m_pLowComplexWriter, item.read, result.correctSequence);
}

// FMIndexWalkProcess.cpp:972-1020
void FMIndexWalkPostProcess::process(const SequenceWorkItemPair& itemPair, const FMIndexWalkResult& result)
{
    if(result.merge) m_mergePassed += 1;
    else if(m_algorithm == FMW_HYBRID && (result.kmerize || result.kmerize2)) {
        if(result.kmerize) m_kmerizePassed += 1;
        else m_qcFail += 1;
        if(result.kmerize2) m_kmerizePassed += 1;
        else m_qcFail += 1;
    } else m_qcFail += 2;
    if(result.merge) {
        const std::string& id = itemPair.first.read.id;
        *m_pCorrectedWriter << ">" << id.substr(0, id.find('/')) << "\n" << result.correctSequence << "\n";      // SeqItem::write
    } else if(m_algorithm == FMW_HYBRID && m_pDiscardWriter != nullptr) {
        writeKmerized(*m_pDiscardWriter, itemPair.first.read, result.correctSequence, result.kmerizedReads);
        writeKmerized(*m_pDiscardWriter, itemPair.second.read, result.correctSequence2, result.kmerizedReads2);
    }
}

} // namespace stride
