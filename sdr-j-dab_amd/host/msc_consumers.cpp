// msc_consumers.cpp -- see msc_consumers.h.
#include "msc_consumers.h"
#include "audio_fir.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dabgpu {

bool check_CRC_bits(uint8_t *in, int16_t size) {
    // CRC-CCITT x^16 + x^12 + x^5 + 1 from all ones over the bits, the received CRC
    // field (last 16 bits) inverted first (dab-constants.h:310-340)
    for (int i = size - 16; i < size; i++) in[i] ^= 1;
    uint32_t reg = 0xFFFF;
    for (int i = 0; i < size; i++) {
        const uint32_t top = (reg >> 15) & 1u;
        reg = (reg << 1) & 0xFFFFu;
        if (top ^ (in[i] & 1u)) reg ^= 0x1021u;
    }
    return reg == 0;
}

// ---- mp2Processor ---------------------------------------------------------------
mp2Processor::mp2Processor(int16_t bitRate, frame_cb cb, FILE *mp2file)
    : cb_(std::move(cb)), mp2File_(mp2file), MP2framesize_(24 * bitRate), MP2frame_(2 * 24 * bitRate, 0) {}

void mp2Processor::addbit(uint8_t b, int16_t nm) {                  // mp2processor.cpp:619-629
    uint8_t byte = MP2frame_[nm / 8];
    const uint8_t bit = (uint8_t)(1u << (7 - (nm & 7)));
    byte = b ? (uint8_t)(byte | bit) : (uint8_t)(byte & ~bit);
    MP2frame_[nm / 8] = byte;
}

void mp2Processor::addtoFrame(uint8_t *v, int16_t amount) {         // mp2processor.cpp:572-617
    const int32_t lf = baudRate_ == 48000 ? MP2framesize_ : 2 * MP2framesize_;
    for (int i = 0; i < amount; i++) {
        if (MP2Header_OK_ == 2) {
            addbit(v[i], MP2bitCount_++);
            if (MP2bitCount_ >= lf) {
                frames_++;
                if (FILE *f = mp2File_.load())
                    (void)std::fwrite(MP2frame_.data(), sizeof(uint8_t), (size_t)lf, f);   // :581-582
                else if (cb_)
                    cb_(MP2frame_.data(), lf, baudRate_);
                MP2Header_OK_ = 0;
                MP2headerCount_ = 0;
                MP2bitCount_ = 0;
            }
        } else if (MP2Header_OK_ == 0) {                            // not in sync yet
            if (v[i] == 1) {
                if (++MP2headerCount_ == 12) {
                    MP2bitCount_ = 0;
                    for (int j = 0; j < 12; j++) addbit(1, MP2bitCount_++);
                    MP2Header_OK_ = 1;
                }
            } else {
                MP2headerCount_ = 0;
            }
        } else if (MP2Header_OK_ == 1) {
            addbit(v[i], MP2bitCount_++);
            if (MP2bitCount_ == 24) {
                // mp2sampleRate (mp2processor.cpp:276-285) + setSamplerate (:262-269)
                static const int32_t rates[8] = {44100, 48000, 32000, 0, 22050, 24000, 16000, 0};
                const uint8_t *f = MP2frame_.data();
                int32_t rate = 0;
                if (f[0] == 0xFF && (f[1] & 0xF6) == 0xF4 && (int)f[2] - 0x10 < 0xE0)
                    rate = rates[(((f[1] & 0x08) >> 1) ^ 4) + ((f[2] >> 2) & 3)];
                if (rate == 48000 || rate == 24000) baudRate_ = rate;
                MP2Header_OK_ = 2;
            }
        }
    }
}

// ---- packet-mode data groups ----------------------------------------------------
static inline uint16_t bits_n(const uint8_t *d, int off, int n) {     // getBits (dab-constants.h:182-190)
    uint16_t r = 0;
    for (int i = 0; i < n; i++) r = (uint16_t)((r << 1) | d[off + i]);
    return r;
}

packetAssembler::packetAssembler(uint8_t DSCTy, uint8_t DGflag, datagroup_cb cb)
    : DSCTy_(DSCTy), DGflag_(DGflag), cb_(std::move(cb)) {}

void packetAssembler::add(uint8_t *data, int16_t length) {
    if (DSCTy_ == 5 && DGflag_) {                                      // handleTDCAsyncstream (:321-339)
        const int16_t packetLength = (int16_t)((bits_n(data, 0, 2) + 1) * 24);
        (void)check_CRC_bits(data, (int16_t)(packetLength * 8));
        return;
    }
    while (true) {                                                     // handlePackets (:221-234)
        const int16_t pLength = (int16_t)((bits_n(data, 0, 2) + 1) * 24 * 8);
        if (length < pLength) return;
        handlePacket(data, length);
        length = (int16_t)(length - pLength);
        if (length < 2) return;
        data = &data[pLength];
    }
}

// avail: bits of the CIF from this packet on.  The reference copies 8 * usefulLength
// bits from bit 24 whatever the packet length (msc-datagroup.cpp:276-283): a CRC-good
// packet whose useful length exceeds it reads on into the next packets, and past the
// CIF's buffer at its end -- here the copy stops at the buffer's end (defined behaviour;
// the same bits wherever the reference's read is defined).
void packetAssembler::handlePacket(uint8_t *data, int avail) {          // msc-datagroup.cpp:241-319
    const int16_t packetLength = (int16_t)((bits_n(data, 0, 2) + 1) * 24);
    const int16_t firstLast = (int16_t)bits_n(data, 4, 2);
    const int16_t address = (int16_t)bits_n(data, 6, 10);
    const int16_t usefulLength = (int16_t)bits_n(data, 17, 7);
    handledPackets_++;
    if (!check_CRC_bits(data, (int16_t)(packetLength * 8))) {
        crcErrors_++;
        return;
    }
    if (address == 0) return;                                          // padding packet
    if (streamAddress_ == -1) streamAddress_ = address;                // the first stream only
    if (streamAddress_ != address) return;
    auto take = [&](bool append) {
        const size_t cur = append ? series_.size() : 0;
        const int n = std::max(0, std::min(8 * (int)usefulLength, avail - 24));
        series_.resize(cur + (size_t)n);
        for (int i = 0; i < n; i++) series_[cur + i] = data[24 + i];
    };
    auto deliver = [&]() {
        datagroups_++;
        if (cb_) cb_(series_);
    };
    if (packetState_ == 0) {                                           // waiting for a start
        if (firstLast == 2) {
            packetState_ = 1;
            take(false);
        } else if (firstLast == 3) {                                   // single packet
            take(false);
            deliver();
        } else {
            series_.resize(0);
        }
    } else {                                                           // within a series
        if (firstLast == 0) {
            take(true);
        } else if (firstLast == 1) {
            take(true);
            deliver();
            packetState_ = 0;
        } else if (firstLast == 2) {                                   // new first: previous lost
            packetState_ = 1;
            take(false);
        } else {
            packetState_ = 0;
            series_.resize(0);
        }
    }
}

// ---- motAssembler -----------------------------------------------------------------
motAssembler::motAssembler(object_cb cb, int32_t max_body_bytes) : cb_(std::move(cb)), maxBody_(max_body_bytes) {}

int32_t motAssembler::entries() const {
    int32_t n = 0;
    for (const element &e : table_) n += e.ordernumber != 0;
    return n;
}

void motAssembler::add_mscDatagroup(const std::vector<uint8_t> &bits) {       // mot-databuilder.cpp:37-95
    const int32_t nbits = (int32_t)bits.size(), nb = nbits / 8;
    if (nbits == 0) return;
    std::vector<uint8_t> g((size_t)nb);
    for (int32_t i = 0; i < nb; i++) {
        uint32_t b = 0;
        for (int k = 0; k < 8; k++) b = (b << 1) | (bits[(size_t)8 * i + k] & 1u);
        g[(size_t)i] = (uint8_t)b;
    }
    auto B = [&](int32_t i) -> uint32_t { return i < nb ? g[(size_t)i] : 0u; };   // fields past the end read 0
    const bool ext = B(0) & 0x80, crcf = B(0) & 0x40, seg = B(0) & 0x20, ua = B(0) & 0x10;
    if (crcf) {                                                           // check_CRC_bits, in int32
        if (nb < 2) return;
        uint32_t reg = 0xFFFF;
        for (int32_t i = 0; i < nb; i++) {
            const uint32_t byte = i >= nb - 2 ? g[(size_t)i] ^ 0xFFu : g[(size_t)i];
            for (int k = 7; k >= 0; k--) {
                const uint32_t top = (reg >> 15) & 1u;
                reg = (reg << 1) & 0xFFFFu;
                if (top ^ ((byte >> k) & 1u)) reg ^= 0x1021u;
            }
        }
        if (reg != 0) return;
    }
    int32_t next = 2 + (ext ? 2 : 0);
    bool last = false, tidf = false;
    uint32_t segno = 0, tid = 0;
    if (seg) {
        last = B(next) >> 7;
        segno = ((B(next) & 0x7Fu) << 8) | B(next + 1);
        next += 2;
    }
    if (ua) {
        tidf = (B(next) >> 4) & 1u;
        const uint32_t li = B(next) & 0xFu;
        next += 1;
        if (tidf) tid = (B(next) << 8) | B(next + 1);
        next += (int32_t)li;
    }
    if (!tidf) return;
    const int32_t dn = std::max(0, nb - next - (crcf ? 2 : 0));
    process_mscGroup(dn ? g.data() + next : g.data(), dn, (uint8_t)(B(0) & 0xFu), last, (int32_t)segno, (uint16_t)tid);
}

motAssembler::element *motAssembler::getHandle(int32_t transportId) {        // mot-data.cpp:590-598
    for (element &e : table_)
        if (e.ordernumber != 0 && e.transportId == transportId) return &e;
    return nullptr;
}

void motAssembler::process_mscGroup(const uint8_t *d, int32_t dn, uint8_t groupType, bool lastSegment,
                                    int32_t segmentNumber, uint16_t transportId) {      // mot-data.cpp:679-728
    const bool hdr = groupType == 3 && segmentNumber == 0;
    if (!hdr && groupType != 4) {                                         // directory mode and the rest
        otherTypes_++;
        return;
    }
    auto B = [&](int32_t i) -> uint32_t { return i >= 0 && i < dn ? d[i] : 0u; };
    const int32_t segmentSize = (int32_t)(((B(0) & 0x1Fu) << 8) | B(1));
    if (dn < 2 || segmentSize + 2 > dn) {
        malformed_++;
        return;
    }
    if (!hdr) {
        if (segmentNumber >= 100) {                                       // the reference writes past marked[100]
            badSegments_++;
            return;
        }
        processSegment(getHandle(transportId), d + 2, segmentNumber, segmentSize, lastSegment);
        return;
    }
    const int32_t headerSize = (int32_t)(((B(5) & 0x0Fu) << 9) | B(6) | (B(7) >> 7));   // (:687-689, d[6] unshifted)
    const int32_t bodySize = (int32_t)((B(2) << 20) | (B(3) << 12) | (B(4) << 4) | (B(5) >> 4));
    if (getHandle(transportId)) return;                                   // processHeader (:56-133)
    auto S = [&](int32_t i) -> uint32_t { return B(i + 2); };
    const int32_t contentType = (int32_t)((S(5) >> 1) & 0x3Fu), contentsubType = (int32_t)(((S(5) & 1u) << 8) | S(6));
    std::string name;
    for (int32_t p = 7; p < headerSize;) {
        const uint32_t PLI = S(p) >> 6, paramId = S(p) & 0x3Fu;
        if (PLI == 0) {
            p += 1;
        } else if (PLI == 1) {
            p += 2;
        } else if (PLI == 2) {
            p += 5;
        } else {
            int32_t length;
            if (S(p + 1) & 0x80u) {
                length = (int32_t)(((S(p + 1) & 0x7Fu) << 8) | S(p + 2));
                p += 3;
            } else {
                length = (int32_t)(S(p + 1) & 0x7Fu);
                p += 2;
            }
            if (paramId == 12)
                for (int32_t i = 0; i < length - 1; i++) name.push_back((char)S(p + i + 1));
            p += length;
        }
    }
    // newEntry (:612-656): the first free entry, else the least ordernumber; the marks stay
    element *e = nullptr;
    for (element &t : table_)
        if (t.ordernumber == 0) {
            e = &t;
            break;
        }
    if (!e) {
        e = &table_[0];
        for (element &t : table_)
            if (t.ordernumber < e->ordernumber) e = &t;
    }
    e->ordernumber = ordernumber_++;
    e->transportId = transportId;
    e->bodySize = bodySize;
    e->contentType = contentType;
    e->contentsubType = contentsubType;
    e->segmentSize = e->numofSegments = -1;
    e->name = name;
    e->tooLarge = bodySize > maxBody_;
    e->body.assign(e->tooLarge ? 0 : (size_t)bodySize, 0);
    if (!lastSegment) processSegment(e, d + 2 + headerSize, 0, segmentSize - headerSize, false);
}

void motAssembler::processSegment(element *h, const uint8_t *segment, int32_t n, int32_t size, bool lastFlag) {   // :278-312
    if (!h || h->tooLarge || size < 0) return;
    if (h->marked[n]) return;
    if (!lastFlag && h->segmentSize == -1) h->segmentSize = size;
    if (h->segmentSize == -1) return;
    if ((int64_t)n * h->segmentSize + size > h->bodySize) return;
    if (size) memcpy(h->body.data() + (size_t)n * h->segmentSize, segment, (size_t)size);
    h->marked[n] = true;
    if (lastFlag) h->numofSegments = n + 1;
    if (h->numofSegments == -1) return;                                   // isComplete (:578-588)
    for (int i = 0; i < h->numofSegments; i++)
        if (!h->marked[i]) return;
    object o;                                                             // handleComplete (:315-336)
    o.kind = h->contentType == 2 ? SLIDE : h->contentType == 7 ? EPG : FILE_;
    if (o.kind == SLIDE) {                                                // show_slide (:337-346)
        if (oldSlide_)
            for (int i = 0; i < h->numofSegments; i++) h->marked[i] = false;
        oldSlide_ = true;
    }
    o.transportId = (uint16_t)h->transportId;
    o.contentType = (uint8_t)h->contentType;
    o.contentsubType = (uint16_t)h->contentsubType;
    o.name = h->name;
    if (o.kind != EPG) o.body = h->body;
    objects_++;
    if (cb_) cb_(o);
}

// ---- ipAssembler: ip_dataHandler (ip-datahandler.cpp:40-127) -----------------------------------
ipAssembler::ipAssembler(datagram_cb on_datagram, quality_cb on_quality)
    : onDatagram_(std::move(on_datagram)), onQuality_(std::move(on_quality)) {}

ipAssembler::result ipAssembler::add_mscDatagroup(const std::vector<uint8_t> &bits) {
    const int32_t nb = (int32_t)(bits.size() / 8);
    std::vector<uint8_t> g((size_t)nb);
    for (int32_t i = 0; i < nb; i++) {
        uint32_t b = 0;
        for (int k = 0; k < 8; k++) b = (b << 1) | (bits[(size_t)8 * i + k] & 1u);
        g[(size_t)i] = (uint8_t)b;
    }
    return add_group(g.data(), nb);
}

ipAssembler::result ipAssembler::add_group(const uint8_t *group, int32_t nbytes) {
    const result r = handle(group, nbytes);
    counts_[r.status]++;
    return r;
}

ipAssembler::result ipAssembler::handle(const uint8_t *g, int32_t nb) {
    if (nb <= 0) return {NOT_ACCEPTED, -1, 0};
    const bool ext = g[0] & 0x80, crcf = g[0] & 0x40, seg = g[0] & 0x20, ua = g[0] & 0x10;
    if (crcf) {                                                           // check_CRC_bits (:54), in int32
        if (nb < 2) return {NOT_ACCEPTED, -1, 0};
        uint32_t reg = 0xFFFF;
        for (int32_t i = 0; i < nb; i++) {
            const uint32_t byte = i >= nb - 2 ? g[i] ^ 0xFFu : g[i];
            for (int k = 7; k >= 0; k--) {
                const uint32_t top = (reg >> 15) & 1u;
                reg = (reg << 1) & 0xFFFFu;
                if (top ^ ((byte >> k) & 1u)) reg ^= 0x1021u;
            }
        }
        if (reg != 0) return {NOT_ACCEPTED, -1, 0};
    }
    // rule 1: bytes past the end read 0; the CRC field reads as check_CRC_bits has left it, inverted
    const int32_t crc0 = crcf ? nb - 2 : nb;
    auto B = [&](int64_t i) -> uint32_t { return i < 0 || i >= nb ? 0u : i >= crc0 ? g[i] ^ 0xFFu : g[i]; };
    int64_t next = 2 + (ext ? 2 : 0);                                     // (:57-74)
    if (seg) next += 2;
    // (a length indicator inside the CRC field leaves next + 2 past the end whichever way it is
    // read: ipLength is 0 then; it is read as stored, as the packet layer's data_offset does)
    if (ua) next += 1 + (int64_t)(next < nb ? g[next] & 0xFu : 0u);
    const int32_t ipLength = (int32_t)((B(next + 2) << 8) | B(next + 3));  // (:79)
    if (!(ipLength < nb)) return {TOO_LONG, -1, ipLength};                // (:80)
    auto D = [&](int32_t i) -> uint32_t { return i < ipLength ? B(next + i) : 0u; };   // ipVector; rule 3
    if (ipLength == 0 || (int8_t)D(0) >> 4 != 4) return {NOT_V4, -1, ipLength};        // rule 2; (:85) a signed char
    const int32_t headerSize = (int32_t)(D(0) & 0xFu);
    int quality = -1;
    if (++handledPackets_ >= 100) {                                       // (:100-104)
        quality = (int16_t)(100 - crcErrors_);
        crcErrors_ = 0;
        handledPackets_ = 0;
        if (onQuality_) onQuality_(quality);
    }
    uint32_t checkSum = 0;
    for (int32_t i = 0; i < 2 * headerSize; i++) checkSum += (D(2 * i) << 8) | D(2 * i + 1);
    checkSum = (checkSum >> 16) + (checkSum & 0xFFFFu);                   // one fold (:107)
    if ((~checkSum & 0xFFFFu) != 0) {
        crcErrors_++;
        return {CHECKSUM, quality, ipLength};
    }
    if (D(9) != 17) return {NOT_UDP, quality, ipLength};                  // (:113-119)
    const int32_t n = ipLength - 4 * headerSize - 8;                      // (:124-127)
    if (n < 0) return {MALFORMED, quality, ipLength};
    std::vector<uint8_t> payload((size_t)n);
    for (int32_t i = 0; i < n; i++) payload[(size_t)i] = (uint8_t)D(4 * headerSize + 8 + i);
    if (onDatagram_) onDatagram_(payload.data(), n);
    return {DELIVERED, quality, ipLength};
}

// ---- padAssembler: padHandler (pad-handler.cpp) ------------------------------------------------
padAssembler::padAssembler(label_cb on_label, datagroup_cb on_group)
    : onLabel_(std::move(on_label)), onGroup_(std::move(on_group)), buffer_(8192, 0) {}

void padAssembler::processAU(const uint8_t *au, int32_t nbytes, int32_t aac_frame_length) {
    if (aac_frame_length < 0) return;
    c_.aus++;
    const int32_t n = std::min(nbytes, aac_frame_length);
    auto B = [&](int32_t i) -> uint8_t { return i < n ? au[i] : 0; };     // theAU is zeroed before the copy
    if (((B(0) >> 5) & 7) != 4) return;                                   // (mp4processor.cpp:264)
    uint8_t pad[255];
    const int32_t count = B(1);
    for (int32_t i = 0; i < count; i++) pad[i] = B(2 + i);
    processPAD(pad, count);
}

static const int32_t kPadSubfield[8] = {4, 6, 8, 12, 16, 24, 32, 48};    // mapLength (:86-95)

void padAssembler::processPAD(const uint8_t *b, int32_t count) {
    c_.pads++;
    touched_ = 0;
    auto done = [&]() {
        for (int k = 0; k < 4; k++) c_.undefined[k] += (touched_ >> k) & 1;
    };
    if (count < 2) {                                                      // rule 1
        touched_ |= 1;
        return done();
    }
    auto rd = [&](int32_t i) -> uint8_t {                                 // rule 2
        if (i < 0) {
            touched_ |= 2;
            return 0;
        }
        return b[i];
    };
    if (((b[count - 2] >> 6) & 3) != 0) return done();                    // only F-PAD type 0
    const int x_padInd = (b[count - 2] >> 4) & 3;
    if (x_padInd == 1) {                                                  // handle_shortPAD (:73-82)
        const uint8_t CI = rd(count - 3);
        uint8_t data[4] = {rd(count - 4), rd(count - 5), rd(count - 6), 0};
        if ((CI & 037) == 2 || (CI & 037) == 3) dynamicLabel(data, 3, CI);
        return done();
    }
    if (x_padInd != 2 || !((b[count - 1] >> 1) & 1)) return done();       // handle_variablePAD (:97-173), CI flag 0
    int32_t base = count - 3, n_ci = 0;
    uint8_t CI_table[4];
    while ((rd(base) & 037) != 0 && n_ci < 4) CI_table[n_ci++] = rd(base--);
    if (n_ci < 4) base -= 1;
    for (int32_t i = 0; i < n_ci; i++) {
        const uint8_t appType = CI_table[i] & 037;
        const int32_t length = kPadSubfield[CI_table[i] >> 5];
        if (appType == 1) {
            const uint8_t byte_0 = rd(base), byte_1 = rd(base - 1);
            rd(base - 2);                                                 // (the reference reads a crc it does not use)
            rd(base - 3);
            length_ = ((byte_0 & 077) << 8) | byte_1;
            index_ = 0;
            base -= 4;
            lastAppType_ = 1;
            lastSet_ = true;
            continue;
        }
        if (appType != 2 && appType != 3 && appType != 12 && appType != 13) {
            lastAppType_ = appType;
            lastSet_ = true;
            c_.unhandled++;
            return done();
        }
        uint8_t data[49];
        for (int32_t j = 0; j < length; j++) data[j] = rd(base - j);
        data[length] = 0;
        if (appType == 2 || appType == 3) {
            dynamicLabel(data, length, CI_table[i]);
        } else {
            if (!lastSet_) touched_ |= 4;                                 // rule 3: last_appType is read
            if ((appType == 12 && lastAppType_ == 1) || (appType == 13 && (lastAppType_ == 12 || lastAppType_ == 13)))
                add_MSC_element(data, length);
        }
        lastAppType_ = appType;
        lastSet_ = true;
        base -= length;
        if (base < 0 && i < n_ci - 1) return done();
    }
    done();
}

void padAssembler::append(const uint8_t *piece, int32_t n) {
    if (!charSetSet_) touched_ |= 4;                                      // rule 3: charSet is read
    if (text_.nbytes + n > 256 || text_.n_pieces + 1 > 64) {              // rule 4
        touched_ |= 8;
        text_.truncated = true;
    }
    for (int32_t i = 0; i < n && text_.text.size() < 256; i++) text_.text.push_back(piece[i]);
    if (text_.piece_len.size() < 64) text_.piece_len.push_back((uint8_t)n);
    text_.nbytes += n;
    text_.n_pieces++;
}

void padAssembler::dynamicLabel(const uint8_t *data, int32_t length, uint8_t CI) {
    auto show = [&]() {
        c_.labels++;
        text_.charset = charSet_;
        if (onLabel_) onLabel_(text_);
    };
    if ((CI & 037) == 2) {                                                // start of segment
        const uint16_t prefix = (uint16_t)((data[0] << 8) | data[1]);
        const int32_t field_1 = (prefix >> 8) & 017;
        const bool Cflag = (prefix >> 12) & 1, first = (prefix >> 14) & 1, last = (prefix >> 13) & 1;
        if (first) {
            charSet_ = (prefix >> 4) & 017;
            charSetSet_ = true;
            text_ = label();
        }
        if (Cflag) {                                                      // the clear command: moreXPad stays as it was
            text_ = label();
            return;
        }
        const int32_t totalDataLength = field_1 + 1;
        int32_t dataLength;
        if (length - 2 < totalDataLength) {
            dataLength = length - 2;
            moreXPad_ = true;
        } else {
            dataLength = totalDataLength;
            moreXPad_ = false;
        }
        append(data + 2, dataLength);
        if (last) {
            if (!moreXPad_)
                show();
            else
                isLastSegment_ = true;
        } else {
            isLastSegment_ = false;
        }
        remainDataLength_ = totalDataLength - dataLength;
    } else if ((CI & 037) == 3 && moreXPad_) {
        int32_t dataLength;
        if (remainDataLength_ > length) {
            dataLength = length;
            remainDataLength_ -= length;
        } else {
            dataLength = remainDataLength_;
            moreXPad_ = false;
        }
        append(data, dataLength);
        if (!moreXPad_ && isLastSegment_) show();
    }
}

void padAssembler::add_MSC_element(const uint8_t *data, int32_t length) {
    if (index_ < 0) {                                                     // rule 3: no length indicator yet
        touched_ |= 4;
        return;
    }
    if (index_ + length >= 8192) {
        c_.guard_dropped++;
        return;
    }
    for (int32_t i = 0; i < length; i++) buffer_[(size_t)index_++] = data[i];
    hiwater_ = std::max(hiwater_, index_);
    if (index_ < length_) return;
    build_MSC_segment(length_);
    index_ = 0;
}

void padAssembler::build_MSC_segment(int32_t length) {
    auto H = [&](int32_t i) -> uint8_t {                                  // rule 3: a byte nothing ever wrote reads 0
        if (i >= hiwater_) touched_ |= 4;
        return buffer_[(size_t)i];
    };
    datagroup g;
    const uint8_t b0 = H(0);
    H(1);
    g.groupType = b0 & 0xF;
    g.extension = b0 & 0x80;
    g.crc = b0 & 0x40;
    g.segment = b0 & 0x20;
    g.user_access = b0 & 0x10;
    bool good = true;
    if (g.crc) {
        if (length < 2) {                                                 // rule 3
            touched_ |= 4;
            good = false;
        } else {                                                          // pad_crc (:360-381)
            uint16_t acc = 0xFFFF;
            for (int32_t i = 0; i < length - 2; i++) {
                acc ^= (uint16_t)(buffer_[(size_t)i] << 8);
                for (int j = 0; j < 8; j++) acc = (acc & 0x8000) ? (uint16_t)((acc << 1) ^ 0x1021) : (uint16_t)(acc << 1);
            }
            good = (uint16_t)~((buffer_[(size_t)length - 2] << 8) | buffer_[(size_t)length - 1]) == acc;
        }
        if (!good) c_.crc_failed++;
    }
    int32_t index = g.extension ? 4 : 2;
    if (g.segment) {
        g.last = H(index) & 0x80;
        g.segmentNumber = (uint16_t)(((H(index) & 0x7F) << 8) | H(index + 1));
        index += 2;
    }
    if (g.user_access) {
        g.lengthInd = H(index) & 0x0F;
        if (H(index) & 0x10) {
            g.transportId = (uint16_t)((H(index + 1) << 8) | H(index + 2));
            index += 3 + (g.lengthInd - 2);
        } else {
            g.transport = false;                                          // "sorry no transportId"
        }
    }
    g.accepted = good && (g.groupType == 3 || g.groupType == 4) && g.transport;
    g.data_offset = index;
    g.data_nbytes = std::max(0, length - index - (g.crc ? 2 : 0));
    g.bytes.assign(buffer_.begin(), buffer_.begin() + length);
    g.data.assign(buffer_.begin() + index, buffer_.begin() + index + g.data_nbytes);
    c_.groups++;
    if (onGroup_) onGroup_(g);
}

// ---- audioResampler -------------------------------------------------------------
// (this file is built with contraction off: a fused multiply-add would round once where the
// reference rounds twice)
const float *audioResampler::kernels() {
    static const struct table {
        float k[15];
        table() { audio_fir_kernels(k); }
    } t;
    return t.k;
}

audioResampler::audioResampler() {
    for (int r = 0; r < 3; r++) f_[r].k = kernels() + 5 * r;
}

// LowPassFIR::Pass (DSPCOMPLEX) (fir-filters.cpp:78-92): the newest sample times k[0] first; each
// term the complex product with (k[i], 0) as the compiler spells it out
audioResampler::pair audioResampler::fir::pass(pair z) {
    pair tmp{0.0f, 0.0f};
    buf[ip] = z;
    for (int i = 0; i < 5; i++) {
        const pair &b = buf[ip - i < 0 ? ip - i + 5 : ip - i];
        const float re = b.re * k[i] - b.im * 0.0f, im = b.re * 0.0f + b.im * k[i];
        tmp.re += re;
        tmp.im += im;
    }
    ip = (ip + 1) % 5;
    return tmp;
}

bool audioResampler::audioOut(const int16_t *V, int32_t amount, int32_t rate, std::vector<float> &out) {
    if (amount < 0) return false;
    const int r = rate == 16000 ? 0 : rate == 24000 ? 1 : rate == 32000 ? 2 : -1;
    if (r == 2 && (amount & 1)) return false;
    const int zeros = r == 1 ? 1 : 2;           // zero pairs after each input pair
    int32_t n = 0;                              // Pass results of this call
    for (int32_t i = 0; i < amount; i++) {
        const pair z{(float)((float)V[2 * i] / 32767.0), (float)((float)V[2 * i + 1] / 32767.0)};
        if (r < 0) {                            // audioOut_48000, the default: label
            out.push_back(z.re);
            out.push_back(z.im);
            continue;
        }
        for (int j = 0; j <= zeros; j++, n++) {
            const pair y = f_[r].pass(j == 0 ? z : pair{0.0f, 0.0f});
            if (r == 2 && (n & 1)) continue;    // audioOut_32000 keeps buffer_1 [2 * i]
            out.push_back(y.re);
            out.push_back(y.im);
        }
    }
    return true;
}

}  // namespace dabgpu
