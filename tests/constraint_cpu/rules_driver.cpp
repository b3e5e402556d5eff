// tests/constraint_cpu/rules_driver.cpp -- CPU test harness for constrained decoding on the host (not part of the product). One translation unit = the test double
// of the compute layer (tests/hostloop_cpu/fake_device.cpp) and the batch harness (batch_driver.cpp), both UNCHANGED, next to whisper_amd/host/batchScheduler.cpp:
//   cc_rules      optionRules::checkConstraint through Whisper::setBatchDecodingConstraint on a runner over the double, with the device entry (batchConstraint.h)
//                 installed -- a hook that records what it is handed -- or left null;
//   cc_automaton  host/phraseAutomaton.h on a phrase list, as JSON, for the comparison with api.compile_phrases.
#include "../hostloop_cpu/fake_device.cpp"
#include "../hostloop_cpu/batch_driver.cpp"
#include "batchConstraint.h"
#include "phraseAutomaton.h"

namespace Whisper
{
	HRESULT setBatchDecodingConstraint( iBatchRunner* runner, const sDecodingConstraint* constraint );	// batchScheduler.cpp
}

namespace
{
	std::string g_ccOut;
	int hookConstraint( wh_context*, const wh_constraint* ) { return 0; }
}

// One call on a fresh runner: states x classes entries all `fill` except entry `at` = `value` (at < 0: none), class `cls` for byte 0, the start, the penalty;
// states == 0 passes nullptr. hook: install the device entry or leave it null. Returns the HRESULT.
extern "C" __attribute__( ( visibility( "default" ) ) ) int cc_rules( const char* modelPath, int hook, uint32_t states, uint32_t classes, uint32_t start, int32_t fill,
	int at, int32_t value, int cls, float penalty )
{
	Whisper::g_batchConstraint = hook ? &hookConstraint : nullptr;
	std::shared_ptr<LoadedModel> lm = std::make_shared<LoadedModel>();
	HRESULT hr = loadVocabulary( modelPath, lm->vocab );
	if( FAILED( hr ) ) return hr;
	void* w = ref_init( modelPath );
	if( !w ) return E_FAIL;
	int32_t h[ 11 ];
	ref_hparams( w, h );
	ref_free( w );
	lm->hp = wh_hparams{ h[ 0 ], h[ 1 ], h[ 2 ], h[ 3 ], h[ 4 ], h[ 5 ], h[ 6 ], h[ 7 ], h[ 8 ], h[ 9 ], h[ 10 ] };
	lm->gpu = fake_model_create( modelPath, 1 );
	TestModel model( lm );
	const sBatchSetup setup{ 2, 1, 0, 0 };
	iBatchRunner* runner = nullptr;
	hr = createBatchRunner( &model, &setup, &runner );
	if( FAILED( hr ) ) return hr;
	std::vector<int32_t> trans( (size_t)states * classes, fill );
	if( at >= 0 && (size_t)at < trans.size() ) trans[ (size_t)at ] = value;
	std::vector<uint8_t> classOf( 256, 0 ), accept( states ? states : 1, 1 );
	classOf[ 0 ] = (uint8_t)cls;
	const sDecodingConstraint k{ states, classes, start, classOf.data(), trans.data(), accept.data(), penalty };
	hr = setBatchDecodingConstraint( runner, states ? &k : nullptr );
	runner->Release();
	return hr;
}

// phrases: '\n'-separated. lead 0 optional, 1 always, 2 never. cc_result() = {"class_of":[...],"trans":[[...]],"accept":[...]} or {"error":"..."}
extern "C" __attribute__( ( visibility( "default" ) ) ) void cc_automaton( const char* phrases, int lead, int repeat )
{
	std::vector<std::string> list;
	std::istringstream in( phrases );
	for( std::string line; std::getline( in, line ); ) list.push_back( line );
	phraseAutomaton::Dfa d;
	std::string why;
	std::ostringstream o;
	if( !phraseAutomaton::compile( list, (phraseAutomaton::eLeadingSpace)lead, repeat != 0, d, why ) ) o << "{\"error\":\"" << why << "\"}";
	else
	{
		o << "{\"class_of\":[";
		for( size_t i = 0; i < 256; i++ ) o << ( i ? "," : "" ) << (int)d.classOf[ i ];
		o << "],\"trans\":[";
		for( uint32_t s = 0; s < d.states; s++ )
		{
			o << ( s ? ",[" : "[" );
			for( uint32_t c = 0; c < d.classes; c++ ) o << ( c ? "," : "" ) << d.trans[ (size_t)s * d.classes + c ];
			o << "]";
		}
		o << "],\"accept\":[";
		for( uint32_t s = 0; s < d.states; s++ ) o << ( s ? "," : "" ) << (int)d.accept[ s ];
		o << "]}";
	}
	g_ccOut = o.str();
}
extern "C" __attribute__( ( visibility( "default" ) ) ) const char* cc_result() { return g_ccOut.c_str(); }
