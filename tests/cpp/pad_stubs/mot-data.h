// Stand-in for the MOT handler: hands on what padHandler::build_MSC_segment hands over.
#ifndef PAD_STUB_MOT_DATA
#define PAD_STUB_MOT_DATA
#include <stdint.h>
class RadioInterface;
// defined by the driver: it records the call and the group buffer as they are at the call
void pad_mot_call(const uint8_t *data, int groupType, int lastSegment, int segmentNumber, int transportId);
class motHandler {
public:
    motHandler(RadioInterface *) {}
    void process_mscGroup(uint8_t *data, uint8_t groupType, bool lastSegment, int16_t segmentNumber, uint16_t transportId) {
        pad_mot_call(data, groupType, lastSegment, segmentNumber, transportId);
    }
};
#endif
