// fib_processor.h -- the FIG parser and service database behind a functional
// drop-in ficHandler: fib_processor of sdr-j-dab
// (includes/backend/fib-processor.h, src/backend/fib-processor.cpp), without Qt.
//
// Host code, scalar and tiny: for one stream a FIB is 30 bytes of FIGs, twelve a frame.
// For many ensembles at once the same parse runs on the GPU, one wave per database
// (dabgpu_fib_parse, csrc/k_fib.hip), and this class is its definition and its host
// end: export_db / import_db speak the library's dabgpu_fic_db record, so the lookups
// below answer from a database the GPU built.  It consumes the CRC-good FIBs the GPU FIC
// decoder delivers (ficHandler / ensembleDecoder::on_fib) and answers the service
// lookups that configure the MSC decoder (kindofService, dataforAudioService,
// dataforDataService).
// The overrun rule (dabgpu.h, dabgpu_fib_parse): a read at or past bit 256 of a FIB reads
// 0, control flow otherwise the reference's; process_FIB works on a zero-extended copy.
//
// Parsed as the reference does (same bit positions, same tables, same quirks):
//   FIG 0/1  sub-channel organisation (short form via the UEP table, long form EEP
//            A/B with the reference's bit-rate formulas)          fib-processor.cpp:278-354
//   FIG 0/2  service organisation (audio TMid 0, packet TMid 3)    :356-422, 1077-1140
//   FIG 0/3  packet-mode service components                        :424-453
//   FIG 0/14 FEC scheme (the reference matches ficList[i].SubChId, which FIG 0/1
//            never sets: only sub-channel id 0 takes effect, for every entry)  :688-705
//   FIG 0/17 programme type and language                           :726-752
//   FIG 0/16 programme number: only its service-table side effect (a new entry per
//            unknown SId, which orders later lookups)              :707-724
//   FIG 1/0  ensemble label, FIG 1/1 service label, FIG 1/5 data service label
//            (" (data)" appended)                                  :850-997
//   FIG 2/5  data service label, as FIG 1/5 without the suffix     :998-1037
// clearEnsemble keeps a service entry's language and programme type, as the
// reference's does (:1149-1163): an entry reused for a new service without FIG 0/17
// reports the old values.
// Labels are converted from the EBU Latin repertoire (charsets.cpp) or taken as
// UTF-8 (charset 15) and returned as UTF-8 strings, 16 characters as transmitted
// (trailing spaces included: the reference compares the full label).
// The remaining FIG 0 extensions (0, 5, 6, 8, 9, 10, 13, 18, 19, 21, 22) carry
// nothing the service lookups read and are skipped.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace dabgpu {

// dab-constants.h:75-77
constexpr uint8_t UNKNOWN_SERVICE = 0100;
constexpr uint8_t AUDIO_SERVICE = 0101;
constexpr uint8_t PACKET_SERVICE = 0102;

// dab-constants.h:152-177
struct packetdata {
    int16_t subchId;
    int16_t startAddr;
    uint8_t uepFlag;
    int16_t protLevel;
    int16_t DSCTy;
    int16_t length;
    int16_t bitRate;
    int16_t FEC_scheme;
    int16_t DGflag;
    int16_t packetAddress;
};
struct audiodata {
    int16_t subchId;
    int16_t startAddr;
    uint8_t uepFlag;
    int16_t protLevel;
    int16_t length;
    int16_t bitRate;
    int16_t ASCTy;
    int16_t language;
    int16_t programType;
};
// one sub-channel of fib_processor::subchannels(): the fields and layout of dabgpu_subch
// (dabgpu.h; this header stands without the GPU library's), flags bit 0 = DABGPU_SUBCH_DABPLUS
struct fib_subch {
    int16_t startAddr, length, bitRate, protLevel, uepFlag, flags;
};

// The database as a plain record: the fields and layout of dabgpu_fic_db (dabgpu.h; this
// header stands without the GPU library's, the drop-in ties the two with a static_assert).
// All zero is a new fib_processor; a free service entry has serviceId 0 and a component
// never bound has service 0 (the class's -1 in both is never read).
struct fib_db {
    struct subch {
        int16_t SubChId, StartAddr, Length, uepFlag, protLevel, BitRate, FEC_scheme;
        uint8_t inUse, reserved;
    } sub[64];
    struct component {
        uint8_t inUse;
        int8_t TMid;
        int16_t service, componentNr, ASCTy, PS_flag, subchannelId;
        uint16_t SCId;
        uint8_t CAflag;
        int8_t DGflag;
        int16_t DSCTy, packetAddress;
    } components[64];
    struct service {
        int32_t serviceId;
        uint8_t inUse, hasName, hasLanguage, charset;
        int16_t language, programType;
        uint8_t data_suffix, reserved[3];
        uint8_t label[16];
    } services[64];
    int32_t EId;
    uint8_t charset, named, reserved[2];
    uint8_t label[16];
    uint8_t reserved2[8];
    struct {                                   // dabgpu_fic_table: the last dabgpu_fib_parse call's (export_db leaves it alone)
        int32_t n, reserved[3];
        fib_subch sub[64];
        uint8_t ids[64];
    } table;
};

class fib_processor {
public:
    // stand-ins for the Qt signals nameofEnsemble / addtoEnsemble
    using ensemble_cb = std::function<void(uint32_t EId, const std::string &name)>;
    using service_cb = std::function<void(const std::string &label)>;
    fib_processor();
    void on_ensemble(ensemble_cb f) { ens_cb_ = std::move(f); }
    void on_service(service_cb f) { svc_cb_ = std::move(f); }
    // both signals as a dabgpu_fic_event carries them: kind 1 nameofEnsemble (id: EId), kind 2
    // addtoEnsemble (id: the service's slot), with the 16 label bytes as transmitted
    using event_cb = std::function<void(int kind, int32_t id, const uint8_t *raw, int charset)>;
    void on_event(event_cb f) { ev_cb_ = std::move(f); }

    // fib: 256 bits, one per byte (as ficHandler hands them over); fib number unused
    void process_FIB(const uint8_t *fib, uint16_t ficno);
    void setupforNewFrame();
    void clearEnsemble();
    uint8_t kindofService(const std::string &label);
    // false (and *d untouched) where the reference returns without filling it in
    bool dataforAudioService(const std::string &label, audiodata *d);
    bool dataforDataService(const std::string &label, packetdata *d);

    // The FIG 0/1 sub-channels seen since clearEnsemble, ordered by SubChId, as the table
    // dabgpu_pipe_set_subch takes: startAddr, length, bitRate, protLevel and uepFlag as the
    // parser stores them; flags = DABGPU_SUBCH_DABPLUS where a bound audio component
    // (FIG 0/2) on the sub-channel has ASCTy 63.  ids (optional) receives each entry's SubChId.
    // classic_audio: also flag DABGPU_SUBCH_MP2 (4) where such a component has ASCTy 0
    // (MPEG layer II, what the reference hands to mp2Processor).
    // packet_data: also flag DABGPU_SUBCH_PACKET (8) where a packet-mode component (TMid 3, FIG
    // 0/2 + FIG 0/3) lies on the sub-channel, unless it has DSCTy 5 with the DG flag set
    // (handleTDCAsyncstream: nothing to deliver).  A component counts once its FIG 0/3 has
    // arrived, which is taken from DSCTy != 0: until then its sub-channel field still holds 0
    // and would flag sub-channel 0; a component announced with DSCTy 0 (unspecified data) is
    // therefore not flagged either.  The audio layers win on a conflict.
    // mot: flag DABGPU_SUBCH_PACKET | DABGPU_SUBCH_MOT (8 | 16) where such a component has DSCTy
    // 60 (MOT: what mscDatagroup hands to mot_databuilder, msc-datagroup.cpp:82-84), whether
    // packet_data is set or not.
    // ip: flag DABGPU_SUBCH_PACKET | DABGPU_SUBCH_IP (8 | 64) where such a component has DSCTy 59
    // (embedded IP: what mscDatagroup hands to ip_dataHandler), whether packet_data is set or not.
    std::vector<fib_subch> subchannels(std::vector<int> *ids = nullptr, bool classic_audio = false,
                                       bool packet_data = false, bool mot = false,
                                       bool pad = false,          // pad: DAB+ entries also get DABGPU_SUBCH_PAD (32)
                                       bool ip = false) const;

    // to and from the public record; import_db rebuilds the UTF-8 labels with label_text.
    // export_db writes everything but db->table.
    void export_db(fib_db *db) const;
    void import_db(const fib_db &db);
    // the last process_FIB met the overrun rule
    bool overran() const { return overrun_; }
    // toQStringUsingCharset (charsets.cpp:69-95) for n label bytes
    static std::string label_text(const uint8_t *bytes, int n, int charset);

    std::string ensembleName() const { return ensemble_; }
    std::vector<std::string> serviceLabels() const;

private:
    struct service {
        int32_t serviceId = -1;
        std::string label;
        uint8_t raw[16] = {}, charset = 0;     // the label as transmitted (export_db)
        bool data_suffix = false;
        bool hasName = false, inUse = false, hasLanguage = false;
        int16_t language = 0, programType = 0;
    };
    struct component {
        bool inUse = false;
        int8_t TMid = 0;
        int service = -1;                      // index into services_
        int16_t componentNr = 0, ASCTy = 0, PS_flag = 0, subchannelId = 0;
        uint16_t SCId = 0;
        uint8_t CAflag = 0;
        int16_t DSCTy = 0;
        int8_t DGflag = 0;
        int16_t packetAddress = 0;
    };
    struct subchannel {
        int32_t SubChId = 0, StartAddr = 0, Length = 0, uepFlag = 0, protLevel = 0, BitRate = 0;
        int16_t language = 0, FEC_scheme = 0;
        bool inUse = false;                    // a FIG 0/1 described it (subchannels())
    };
    uint32_t bits(const uint8_t *d, int off, int n);   // with the overrun rule's bookkeeping
    void fig0(const uint8_t *d);
    void fig1(const uint8_t *d);
    int fig0_1(const uint8_t *d, int used);
    int fig0_2(const uint8_t *d, int used, int pd);
    int fig0_3(const uint8_t *d, int used);
    void fig0_14(const uint8_t *d);
    void fig0_16(const uint8_t *d);
    void fig0_17(const uint8_t *d);
    void fig2(const uint8_t *d);
    int find_service(int32_t sid);
    int find_packet_component(int16_t scid) const;
    int bind(int8_t TMid, int32_t sid, int16_t compnr);
    int lookup(const std::string &label) const;       // first named service with this label

    service services_[64];
    component components_[64];
    subchannel sub_[64];
    std::string ensemble_;
    uint32_t eid_ = 0;
    uint8_t ens_raw_[16] = {}, ens_charset_ = 0;
    bool firstTime_ = true;
    const uint8_t *fib_end_ = nullptr;         // one past bit 255 of the copy process_FIB walks
    bool overrun_ = false;
    ensemble_cb ens_cb_;
    service_cb svc_cb_;
    event_cb ev_cb_;
};

}  // namespace dabgpu
