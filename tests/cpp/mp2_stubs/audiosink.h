// Stand-in for the sound-card sink: keeps what the decoder hands over.
#ifndef MP2_STUB_AUDIOSINK
#define MP2_STUB_AUDIOSINK
#include <stdint.h>
#include <vector>
class audioSink {
public:
    std::vector<int16_t> pcm;        // 2 * amount values per call
    std::vector<int32_t> rate;       // one per call
    void audioOut(int16_t *v, int32_t amount, int32_t r) {
        pcm.insert(pcm.end(), v, v + 2 * amount);
        rate.push_back(r);
    }
};
#endif
