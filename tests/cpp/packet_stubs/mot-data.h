// Stand-in for the MOT handler: keeps what mot_databuilder::add_mscDatagroup hands over.
#ifndef PACKET_STUB_MOT_DATA
#define PACKET_STUB_MOT_DATA
#include <stdint.h>
#include <vector>
class RadioInterface;
struct motCall {
    int32_t groupType, lastSegment, segmentNumber, transportId;
};
extern std::vector<motCall> mot_calls;
class motHandler {
public:
    motHandler(RadioInterface *) {}
    void process_mscGroup(uint8_t *, uint8_t groupType, bool lastSegment, int16_t segmentNumber, uint16_t transportId) {
        mot_calls.push_back({groupType, lastSegment, segmentNumber, transportId});
    }
};
#endif
