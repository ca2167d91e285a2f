// msc_consumers.h -- what the reference does with the decoded MSC bits of a
// subchannel, minus the codecs: the plug-in interfaces (dabVirtual, dabProcessor),
// the MPEG-1/2 layer II frame synchroniser of mp2Processor (mp2processor.cpp:572-629),
// the packet-mode data-group assembly of mscDatagroup (msc-datagroup.cpp:221-339),
// motHandler's header mode (mot-data.cpp:679-728), ip_dataHandler (ip-datahandler.cpp) and
// audioSink's conversion to 48 kHz floats (audiosink.cpp:235-360).
// Host code (a few bit operations per decoded bit, after the GPU's Viterbi): no Qt,
// no kjmp2 / faad / sockets -- complete frames, data groups, MOT objects and UDP payloads go to
// callbacks instead.  Same state machines and quirks as the reference.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

namespace dabgpu {

// dabProcessor (includes/backend/audio/dab-processor.h): addtoFrame(bits, nbits),
// one bit per byte as the deconvolver delivers them
class dabProcessor {
public:
    virtual ~dabProcessor() = default;
    virtual void addtoFrame(uint8_t *v, int16_t nbits) { (void)v; (void)nbits; }
    // mp2Processor::setFile (mp2processor.cpp:631-633); the other processors ignore it
    virtual void setFile(FILE *f) { (void)f; }
};

// dabVirtual (includes/backend/dab-virtual.h:36-47): a subchannel's CIF fragments
class dabVirtual {
public:
    virtual ~dabVirtual() = default;
    virtual int32_t process(int16_t *v, int16_t cnt) { (void)v; (void)cnt; return 0; }
    virtual void stopRunning() {}
    virtual void stop() {}
    // dab-virtual.h:43: the mp2 / mp4 dump files (dabConcurrent hands the mp2 file to an
    // mp2Processor, dab-concurrent.cpp:196-200; the mp4 file is never written in v0.997)
    virtual void setFiles(FILE *mp2, FILE *mp4) { (void)mp2; (void)mp4; }
};

// check_CRC_bits (dab-constants.h:310-340): CRC-16 over size bits (1 per byte) whose
// last 16 are the inverted CRC; inverts those 16 bits in place, as the reference does
bool check_CRC_bits(uint8_t *in, int16_t size);

// mp2Processor::addtoFrame (mp2processor.cpp:572-629): sync on 12 consecutive 1 bits,
// read the 24-bit header (sample rate: 48 or 24 kHz, else unchanged), collect the frame
// (24 * bitRate bits at 48 kHz, twice that at 24 kHz) and hand it over -- where the
// reference writes it to the mp2 file or decodes it with kjmp2.  With a file set
// (setFile, mscHandler::setFiles) the frame is written INSTEAD of handed to the callback,
// exactly as mp2processor.cpp:581-586 writes instead of decoding -- including the
// reference's count: fwrite of lf BYTES where lf is the frame's length in bits, i.e.
// the frame's lf / 8 bytes followed by the rest of the (2 * 24 * bitRate byte) frame
// buffer, which the reference leaves uninitialised and this class zero-fills.
class mp2Processor : public dabProcessor {
public:
    using frame_cb = std::function<void(const uint8_t *frame, int32_t nbits, int32_t sampleRate)>;
    mp2Processor(int16_t bitRate, frame_cb cb, FILE *mp2file = nullptr);
    void addtoFrame(uint8_t *v, int16_t nbits) override;
    void setFile(FILE *f) override { mp2File_ = f; }
    int32_t sampleRate() const { return baudRate_; }
    int32_t frames() const { return frames_; }
private:
    void addbit(uint8_t b, int16_t nm);
    frame_cb cb_;
    std::atomic<FILE *> mp2File_{nullptr};   // setFile from the GUI thread, read by the decoding thread
    int32_t baudRate_ = 48000;
    int32_t MP2framesize_;                  // bits
    std::vector<uint8_t> MP2frame_;
    int16_t MP2Header_OK_ = 0, MP2headerCount_ = 0, MP2bitCount_ = 0;
    int32_t frames_ = 0;
};

// audioSink::audioOut (audiosink.cpp:235-360) minus the device: int16 stereo PCM at 16, 24, 32 or
// 48 kHz in, the 48 kHz float pairs it puts into _O_Buffer out (appended to `out`).  16, 24 and
// 32 kHz go through LowPassFIR (5, ...)::Pass (fir-filters.cpp:78-92) over the zero-stuffed input,
// 32 kHz keeping every second result of a call; every other rate is scaled only.  The same
// function, bit for bit, as the GPU's audio output layer (dabgpu_audio_out in include/dabgpu.h):
// every product and sum is rounded to float on its own.  The three filters live as long as the
// object; a call at one rate leaves the others as they were.  Not modelled: the ring's
// back-pressure and dumpFile.  An odd amount at 32000 (the reference then puts a float it never
// wrote) and a negative amount deliver nothing and return false.
class audioResampler {
public:
    audioResampler();
    bool audioOut(const int16_t *V, int32_t amount, int32_t rate, std::vector<float> &out);
    // the kernels of f_16000, f_24000 and f_32000 (fir-filters.cpp:35-69), 5 taps each
    static const float *kernels();
private:
    struct pair { float re, im; };
    struct fir {                                // LowPassFIR's Buffer and ip
        pair buf[5] = {};
        int ip = 0;
        const float *k = nullptr;
        pair pass(pair z);
    };
    fir f_[3];                                  // 16000, 24000, 32000
};

// mscDatagroup's packet handling (msc-datagroup.cpp:221-339): the decoded bits of a CIF
// are a sequence of DAB packets (24, 48, 72 or 96 bytes); each is CRC-checked, padding
// packets (address 0) dropped, and the packets of the first address seen are assembled
// into MSC data groups by their first/last flags.  A data group (bits, one per byte) goes
// to the callback that stands in for the DSCTy's data handler (MOT, IP, journaline).
// DSCTy 5 with DGflag set: the transparent data channel of handleTDCAsyncstream, which
// only checks the first packet's CRC.
class packetAssembler {
public:
    using datagroup_cb = std::function<void(const std::vector<uint8_t> &bits)>;
    packetAssembler(uint8_t DSCTy, uint8_t DGflag, datagroup_cb cb);
    void add(uint8_t *data, int16_t length);           // one CIF's decoded bits (24 * bitRate)
    int32_t crcErrors() const { return crcErrors_; }
    int32_t packets() const { return handledPackets_; }
    int32_t datagroups() const { return datagroups_; }
private:
    void handlePacket(uint8_t *data, int avail);
    uint8_t DSCTy_, DGflag_;
    datagroup_cb cb_;
    int16_t packetState_ = 0;
    int32_t streamAddress_ = -1;
    std::vector<uint8_t> series_;
    int32_t crcErrors_ = 0, handledPackets_ = 0, datagroups_ = 0;
};

// motHandler in header mode (mot-data.cpp:679-728: processHeader, processSegment, newEntry,
// getHandle, isComplete, handleComplete, show_slide) behind mot_databuilder::add_mscDatagroup
// (mot-databuilder.cpp:37-95): MSC data groups in, slides and files out through a callback
// where the reference emits the_picture or fopens.  The same function, byte for byte, as the
// GPU's MOT layer (dabgpu_mot_groups in include/dabgpu.h, whose rules 1-6 for what the
// reference leaves undefined hold here too: bytes past a group read 0, segment numbers >= 100
// and malformed groups are dropped and counted, sizes are int32, bodies above max_body_bytes
// are refused, directory mode -- group type 6 -- is counted and ignored).
class motAssembler {
public:
    enum { SLIDE = 1, EPG = 2, FILE_ = 3 };
    struct object {
        int kind;                       // SLIDE, EPG (contentType 7: nothing is delivered, body empty) or FILE_
        uint16_t transportId;
        uint8_t contentType;
        uint16_t contentsubType;
        std::string name;               // the whole name (the GPU record keeps its first 128 bytes)
        std::vector<uint8_t> body;
    };
    using object_cb = std::function<void(const object &)>;
    explicit motAssembler(object_cb cb, int32_t max_body_bytes = 65536);
    // one MSC data group, one bit per byte, as packetAssembler delivers it
    void add_mscDatagroup(const std::vector<uint8_t> &bits);
    // motHandler::process_mscGroup on a data field of nbytes bytes
    void process_mscGroup(const uint8_t *data, int32_t nbytes, uint8_t groupType, bool lastSegment, int32_t segmentNumber,
                          uint16_t transportId);
    int32_t objects() const { return objects_; }
    int32_t malformed() const { return malformed_; }
    int32_t badSegments() const { return badSegments_; }
    int32_t otherTypes() const { return otherTypes_; }
    int32_t entries() const;
private:
    struct element {                    // motElement (mot-data.h:33-44); ordernumber 0: free
        int32_t ordernumber = 0, transportId = 0, bodySize = 0, segmentSize = -1, numofSegments = -1;
        int32_t contentType = 0, contentsubType = 0;
        bool tooLarge = false;
        bool marked[100] = {};
        std::string name;
        std::vector<uint8_t> body;
    };
    element *getHandle(int32_t transportId);
    void processSegment(element *h, const uint8_t *segment, int32_t segmentNumber, int32_t segmentSize, bool lastFlag);
    object_cb cb_;
    int32_t maxBody_;
    element table_[16];
    int32_t ordernumber_ = 1;
    bool oldSlide_ = false;
    int32_t objects_ = 0, malformed_ = 0, badSegments_ = 0, otherTypes_ = 0;
};

// ip_dataHandler (ip-datahandler.cpp:40-127, show_crcErrors on): MSC data groups in, the UDP payload
// of every IPv4 datagram with a good header checksum out through a callback where the reference
// emits writeDatagram, and the number show_ipErrors emits every 100 datagrams through another.  The
// same function, byte for byte, as the GPU's IP layer (dabgpu_ip_groups in include/dabgpu.h, whose
// rules 1-5 for what the reference leaves undefined hold here too: bytes past a group read 0 and a
// datagram over the group's own CRC bytes reads them complemented, ipLength 0 is no IPv4, header
// bytes past ipLength read 0 and a negative payload length is counted as malformed, lengths are
// int32; there is no arena here, so rule 6 has no counterpart).
class ipAssembler {
public:
    enum { DELIVERED = 0, NOT_ACCEPTED, TOO_LONG, NOT_V4, CHECKSUM, NOT_UDP, MALFORMED, NSTATUS };
    struct result {
        int status;                     // what became of the group
        int quality;                    // what show_ipErrors emitted inside the call, else -1
        int32_t ip_bytes;               // ipLength, 0 when the group never got that far
    };
    using datagram_cb = std::function<void(const uint8_t *payload, int32_t nbytes)>;
    using quality_cb = std::function<void(int value)>;
    explicit ipAssembler(datagram_cb on_datagram, quality_cb on_quality = nullptr);
    // one MSC data group, one bit per byte, as packetAssembler delivers it
    result add_mscDatagroup(const std::vector<uint8_t> &bits);
    // ... as bytes, its CRC field as received
    result add_group(const uint8_t *group, int32_t nbytes);
    int32_t handledPackets() const { return handledPackets_; }
    int32_t crcErrors() const { return crcErrors_; }
    void setCounters(int32_t handledPackets, int32_t crcErrors) { handledPackets_ = handledPackets; crcErrors_ = crcErrors; }
    int32_t count(int status) const { return counts_[status]; }
private:
    result handle(const uint8_t *group, int32_t nbytes);
    datagram_cb onDatagram_;
    quality_cb onQuality_;
    int32_t handledPackets_ = 0, crcErrors_ = 0;
    int32_t counts_[NSTATUS] = {};
};

// padHandler (pad-handler.cpp) for one DAB+ stream: the PAD of every good AU whose first
// syntactic element is a data stream element in, dynamic labels and X-PAD MSC data groups out
// through callbacks, where the reference emits showLabel or calls process_mscGroup.  The same
// function, byte for byte, as the GPU's PAD layer (dabgpu_pad_aus in include/dabgpu.h, whose
// rules 1-4 for what the reference leaves undefined hold here too: a PAD shorter than 2 bytes is
// ignored, reads below the PAD give 0, a new handler has last_appType 0, no group in progress,
// charSet 0 and a zeroed group buffer, the label record keeps 256 bytes and 64 pieces).
// dynamicLabel's function-local statics are members.  Charset conversion is the caller's: the
// label is the bytes the reference hands to toQStringUsingCharset, with the piece boundaries.
class padAssembler {
public:
    struct label {
        int32_t charset = 0;
        int32_t nbytes = 0, n_pieces = 0;       // the full counts
        bool truncated = false;
        std::vector<uint8_t> piece_len;         // the first 64
        std::vector<uint8_t> text;              // the first 256 bytes
    };
    struct datagroup {                          // build_MSC_segment's parse (:299-357)
        std::vector<uint8_t> bytes;             // the group, msc_dataGroupLength bytes
        int32_t data_offset = 0, data_nbytes = 0;   // the reference's index; max(0, length - index - CRC bytes)
        bool extension = false, crc = false, segment = false, user_access = false, last = false, transport = true;
        bool accepted = false;                  // handed to process_mscGroup
        uint16_t segmentNumber = 0xFFFF, transportId = 0xFFFF;
        uint8_t groupType = 0, lengthInd = 0;
        std::vector<uint8_t> data;              // what process_mscGroup's pointer shows: the buffer from index, data_nbytes of it
    };
    using label_cb = std::function<void(const label &)>;
    using datagroup_cb = std::function<void(const datagroup &)>;
    padAssembler(label_cb on_label, datagroup_cb on_group);
    // mp4Processor's part (mp4processor.cpp:255-265): au readable for nbytes, aac_frame_length its
    // length (negative: the AU failed its CRC); bytes past the length read 0
    void processAU(const uint8_t *au, int32_t nbytes, int32_t aac_frame_length);
    // padHandler::processPAD on a PAD of count bytes (AU[2 .. 2 + count))
    void processPAD(const uint8_t *pad, int32_t count);
    struct counters {
        int32_t labels = 0, groups = 0, aus = 0, pads = 0, unhandled = 0, undefined[4] = {0, 0, 0, 0}, crc_failed = 0,
                guard_dropped = 0;
    };
    const counters &count() const { return c_; }
private:
    void dynamicLabel(const uint8_t *data, int32_t length, uint8_t CI);
    void append(const uint8_t *piece, int32_t n);
    void add_MSC_element(const uint8_t *data, int32_t length);
    void build_MSC_segment(int32_t length);
    label_cb onLabel_;
    datagroup_cb onGroup_;
    counters c_;
    uint32_t touched_ = 0;                      // rules the current PAD met (bit k-1: rule k)
    int32_t lastAppType_ = 0, index_ = -1, length_ = 0, charSet_ = 0, hiwater_ = 0;
    bool lastSet_ = false, charSetSet_ = false;
    int32_t remainDataLength_ = 0;
    bool isLastSegment_ = false, moreXPad_ = false;
    label text_;
    std::vector<uint8_t> buffer_;
};

}  // namespace dabgpu
